// Neighbourhood verification: the integer box counts behind the fractions skill score (Roberts and Lean 2008), for up to 8 thresholds
// and up to 8 box half-widths at once, per (sample, channel) plane.  include/swv2.h states the definition in full; in short, with
// n_f(h, w) / n_o(h, w) the number of forecast / analysis events in rows max(0, h - r) .. min(H - 1, h + r) and columns w - r .. w + r
// modulo W (the poles clip the box, the longitude wraps; a point with a NaN is no event in either field):
//     rows[B][C][K][S][H][3] = (sum_w (n_f - n_o)^2, sum_w n_f^2, sum_w n_o^2)          int64, exact
// The first stencil of the verification family: two launches behind the one entry point swv2_fss_rows, no float arithmetic on any output.
//
//   launch 1  fss_mask_kernel<K, BASE, BELOW>   8 (12 with a base) B / element, each input read once with 16-byte loads, on the slices
//             and the workgroup index (c * slices + sl) * B + b of plane_stream.h.  The unit of work is one wave on 256 columns of one row
//             (unit u = row * ceil(W / 256) + segment; the waves of a plane take u = 4 sl + wave, + 4 slices, ...): a lane compares its 4
//             points with the K thresholds, the 8 lanes of a 32-column word OR their nibbles together (DPP) and the first of them stores
//             the word.  Out: bits[plane][k][field][H][ceil(W / 32)], column c of a row at bit c & 31 of word c >> 5 (the bits past W are
//             0), field 0 = forecast, 1 = analysis; and the invalid points of the workgroup, inv[plane][sl].  2 K bits per point: 1 / 4
//             (K = 8) to 1 / 32 (K = 1) of what was read, which launch 2 finds in the memory-side cache.
//   launch 2  fss_box_kernel                    one workgroup per (plane, threshold, band of rows): planes * K * ceil(H / band) workgroups,
//             band = swv2_fss_band_rows(planes, H, K, r_max).  For each tile of at most 1024 columns it builds the LDS image of the rows
//             h0 - r_max .. h1 - 1 + r_max of both fields (rows beyond a pole are zeros), each row EXTENDED: image bit j of a row is the
//             column (32 * (c0 >> 5) - 32 + j) mod W, so a window that crosses the date line is plain addressing (fss_ext_word).  A
//             thread owns up to 4 columns, 256 apart.  Per scale r it keeps the box count of each of its columns and both fields in a
//             register and slides it down the band: + the window count of row h + r, - that of row h - r, a window count being the
//             popcount of 2 r + 1 <= 65 bits out of three 32-bit words, or of at most 31 bits out of two (fss_window).  The three terms of a row are summed over the 16
//             lanes of a DPP row and added to the band's accumulators in LDS (64-bit integer ds_add: the order cannot matter); after the
//             last tile the workgroup stores its band of `rows`.  The workgroup (plane, k = 0, band 0) also folds inv[plane][.] into n_invalid[plane].
//
// Bands (fss_band_rows, the one statement of the plan; swv2_fss_band_rows asks it).  Starting a band costs 2 r window counts per column
// and scale, walking it 2 per row: bands are at least max(2 r_max + 1, 32) rows tall (at most 80, the LDS image) so that the start-up
// stays below the walk -- unless that leaves fewer than 8 workgroups (one per XCD), a call too small for that to matter, which is cut
// down to bands of 8 rows to have them.  73 x 2 planes of 720 x 1440, K = 4, r_max = 32: 11 bands of 66 rows, 6424 workgroups of 40 KB LDS.
//
// Integer bounds.  A box count is at most 65 * 65 = 4225 (int).  A squared difference or count is at most 4225^2 = 17 850 625; a thread adds
// at most 4 of them per (row, scale, tile): 7.2e7, and 16 lanes 1.15e9 < 2^32 (uint32_t).  Everything beyond is 64-bit: a row sum at
// W = 16384 is at most 2.9e11.  Counts of invalid points: at most H W < 2^30 (int).
//
// Workspace: uint32_t bits[planes][K][2][H][ceil(W / 32)], int inv[planes][slices].  Every word of it is written by launch 1 before launch 2
// reads it; nothing is zeroed beforehand, every slot of rows and n_invalid has one owner, nothing else is written.
#include "plane_stream.h"

namespace {

constexpr int FSS_MAX_K = 8;
constexpr int FSS_MAX_S = 8;
constexpr int FSS_MAX_R = 32;
constexpr int FSS_BAND_MAX = 80;          // rows of a band: with 2 r_max halo rows, 8 scales and 1024 columns the LDS image is 57 984 B
constexpr int FSS_BAND_TALL = 32;         // a band is at least this tall, or as tall as the largest box ...
constexpr int FSS_BAND_MIN = 8;           // ... unless the call has fewer than FSS_SMALL_WGS workgroups (one per XCD): then at least this
constexpr int FSS_SMALL_WGS = 8;
constexpr int FSS_TILE_COLS = 1024;       // columns of one LDS image: FSS_CPT per thread
constexpr int FSS_CPT = 4;                // ... of a workgroup of 256: fss_box_kernel instantiates the walk for 1 .. FSS_CPT
static_assert(FSS_TILE_COLS == 256 * FSS_CPT && FSS_CPT == 4, "fss_box_kernel picks the walk among NJ = 1 .. 4");

struct fss_scales { int r[FSS_MAX_S]; };

__host__ __device__ inline int fss_words(int W) { return (W + 31) >> 5; }

// the plan: rows per band of `units` (plane, threshold) pairs, bands `tall` rows where the call is large enough and never above `most`
__host__ __device__ inline int fss_bands(long units, int H, int tall, int most) {
    if (tall > most) tall = most;
    long nb = H / tall > 1 ? H / tall : 1;
    if (units * nb < FSS_SMALL_WGS) {
        const long want = (FSS_SMALL_WGS + units - 1) / units, cut = (H + FSS_BAND_MIN - 1) / FSS_BAND_MIN;
        const long n = want < cut ? want : cut;
        if (n > nb) nb = n;
    }
    const int band = (int)((H + nb - 1) / nb);
    return band < most ? band : most;
}
__host__ __device__ inline int fss_tall(int rmax) { return 2 * rmax + 1 > FSS_BAND_TALL ? 2 * rmax + 1 : FSS_BAND_TALL; }
__host__ __device__ inline int fss_band_rows(long planes, int H, int K, int rmax) { return fss_bands(planes * K, H, fss_tall(rmax), FSS_BAND_MAX); }

// column tiles of the box kernel: ceil(W / 1024) tiles of ceil(W / tiles) columns (the last one to W); words per image row: those of the
// widest tile, 32 columns of halo on either side and two words that a window's three-word read may touch behind its last bit
__host__ __device__ inline int fss_tiles(int W, int tile = FSS_TILE_COLS) { return (W + tile - 1) / tile; }
__host__ __device__ inline int fss_tile_cols(int W, int tile = FSS_TILE_COLS) { return (W + fss_tiles(W, tile) - 1) / fss_tiles(W, tile); }
__host__ __device__ inline int fss_stride_of(int tcols) { return (tcols + 63) / 32 + 4; }
__host__ __device__ inline int fss_image_stride(int W, int tile = FSS_TILE_COLS) { return fss_stride_of(fss_tile_cols(W, tile)); }
__host__ __device__ inline size_t fss_lds_bytes(int W, int band, int rmax, int S) {
    return (size_t)band * S * 3 * 8 + (size_t)2 * (band + 2 * rmax) * fss_image_stride(W) * 4;
}

// n <= 32 bits of a bit row from column c on (c + n <= W: no word behind the row is read)
__host__ __device__ inline uint32_t fss_bits(const uint32_t* row, int c, int n) {
    const int i = c >> 5, sh = c & 31;
    uint32_t v = row[i] >> sh;
    if (sh + n > 32) v |= row[i + 1] << (32 - sh);
    return n < 32 ? v & ((1u << n) - 1u) : v;
}

// 32 bits of the periodic extension of a bit row of W columns: bit j = column (cs + j) mod W, for any cs and any W >= 1
__host__ __device__ inline uint32_t fss_ext_word(const uint32_t* row, int W, int cs) {
    int c = cs % W;
    if (c < 0) c += W;
    uint32_t out = 0;
    for (int filled = 0; filled < 32;) {
        const int n = 32 - filled < W - c ? 32 - filled : W - c;
        out |= fss_bits(row, c, n) << filled;
        filled += n;
        c += n;
        if (c == W) c = 0;
    }
    return out;
}

// the masks of a window of len = 2 r + 1 bits: its bits 0 .. 31, 32 .. 63 and (r = 32 alone) bit 64
struct fss_mask3 { uint32_t m0, m1, m2; };
__host__ __device__ inline fss_mask3 fss_window_masks(int r) {
    const int len = 2 * r + 1;
    return {len >= 32 ? ~0u : (1u << len) - 1u, len >= 64 ? ~0u : len > 32 ? (1u << (len - 32)) - 1u : 0u, len > 64 ? 1u : 0u};
}

// bits sh .. sh + 31 of hi : lo, sh < 32 (v_alignbit_b32; the 64-bit shift it stands for compiled to v_lshrrev_b64)
__host__ __device__ inline uint32_t fss_funnel(uint32_t hi, uint32_t lo, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}

// the set bits among the 2 r + 1 image bits from bit s on.  WIDE (r >= 16, up to 65 bits): three words, two funnel shifts, two popcounts
// and the 65th bit; else (at most 31 bits): two words, one funnel shift, one popcount
template <bool WIDE>
__host__ __device__ inline int fss_window(const uint32_t* row, int s, const fss_mask3 m) {
    const int i = s >> 5, sh = s & 31;
    const uint32_t a0 = row[i], a1 = row[i + 1];
    const int n0 = __builtin_popcount(fss_funnel(a1, a0, sh) & m.m0);
    if constexpr (!WIDE) return n0;
    const uint32_t a2 = row[i + 2];
    return n0 + __builtin_popcount(fss_funnel(a2, a1, sh) & m.m1) + (int)((a2 >> sh) & m.m2);
}

// One image word: field f, image row ir (plane row h0 - rmax + ir), word iw of the tile that starts at column c0.
__host__ __device__ inline uint32_t fss_image_word(const uint32_t* field_bits, int H, int W, int h0, int rmax, int c0, int ir, int iw) {
    const int g = h0 - rmax + ir;
    if (g < 0 || g >= H) return 0u;                           // beyond a pole: no events
    return fss_ext_word(field_bits + (size_t)g * fss_words(W), W, 32 * ((c0 >> 5) + iw) - 32);
}

// The walk of one thread (tid of 256) over the band [h0, h1) for one tile [c0, c0 + tc) and one scale: emit(row of the band, d2, f2, o2)
// once per row with the thread's share of the three sums.  imgF / imgO: the images of the two fields, `stride` words per row.
// NJ = ceil(tc / 256): the columns of a thread, 256 apart (the last one may lie beyond the tile: `ok`); WIDE: r >= 16 (fss_window).
template <int NJ, bool WIDE, class Emit>
__host__ __device__ inline void fss_walk(const uint32_t* imgF, const uint32_t* imgO, int stride, int tid, int h0, int h1, int rmax, int c0,
                                         int tc, int r, Emit&& emit) {
    const fss_mask3 m = fss_window_masks(r);
    int s[NJ], nf[NJ], no[NJ];
    bool ok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = c0 + tid + 256 * j;
        ok[j] = c < c0 + tc;
        s[j] = (ok[j] ? c : c0 + tc - 1) + 32 - r - 32 * (c0 >> 5);          // the window's first image bit (a spare thread: the last column's)
        nf[j] = no[j] = 0;
    }
    for (int g = h0 - r; g < h0 + r; ++g) {                   // the box of row h0 without its last row
        const int at = (g - h0 + rmax) * stride;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            nf[j] += fss_window<WIDE>(imgF + at, s[j], m);
            no[j] += fss_window<WIDE>(imgO + at, s[j], m);
        }
    }
    for (int h = h0; h < h1; ++h) {
        const int in = (h + r - h0 + rmax) * stride, out = (h - r - h0 + rmax) * stride;
        uint32_t d2 = 0, f2 = 0, o2 = 0;                      // at most 4 * 4225^2 each
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            nf[j] += fss_window<WIDE>(imgF + in, s[j], m);
            no[j] += fss_window<WIDE>(imgO + in, s[j], m);
            if (ok[j]) {
                const int d = nf[j] - no[j];
                d2 += (uint32_t)(d * d);
                f2 += (uint32_t)(nf[j] * nf[j]);
                o2 += (uint32_t)(no[j] * no[j]);
            }
            nf[j] -= fss_window<WIDE>(imgF + out, s[j], m);
            no[j] -= fss_window<WIDE>(imgO + out, s[j], m);
        }
        emit(h - h0, d2, f2, o2);
    }
}

// all-reduce over lane groups on the vector ALU (DPP; every lane active): OR over 8 lanes, sum over the 16 lanes of a DPP row
template <int CTRL>
__device__ __forceinline__ uint32_t fss_dpp(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t fss_or8(uint32_t v) {
    v |= fss_dpp<0xb1>(v);                                    // quad_perm [1,0,3,2]
    v |= fss_dpp<0x4e>(v);                                    // quad_perm [2,3,0,1]
    v |= fss_dpp<0x141>(v);                                   // row_half_mirror
    return v;
}
__device__ __forceinline__ uint32_t fss_sum16(uint32_t v) {
    v += fss_dpp<0xb1>(v);
    v += fss_dpp<0x4e>(v);
    v += fss_dpp<0x141>(v);
    v += fss_dpp<0x140>(v);                                   // row_mirror
    return v;
}

template <bool BELOW>
__device__ __forceinline__ bool fss_is(float x, float th) { return BELOW ? x < th : x > th; }

template <int K, bool BASE, bool BELOW>
__global__ __launch_bounds__(256) void fss_mask_kernel(const float* __restrict__ prd, long prd_bs, const float* __restrict__ tar, long tar_bs,
                                                       const float* __restrict__ base, const float* __restrict__ thr, long thr_bs,
                                                       uint32_t* __restrict__ bits, int* __restrict__ inv, int B, int C, int H, int W, int slices) {
    const auto [b, c, sl] = plane_shared_index(B, slices);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int WB = fss_words(W), nseg = (W + 255) >> 8;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    const float* p = prd + b * prd_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    const float* bp = BASE ? base + (long)c * plane : nullptr;
    const size_t pl = (size_t)b * C + c;
    uint32_t* out = bits + pl * K * 2 * H * WB;
    float th[K];
#pragma unroll
    for (int k = 0; k < K; ++k) th[k] = thr[b * thr_bs + (long)c * K + k];
    int ninv = 0;
    const int units = H * nseg;                               // <= H W / 4
    for (int u = sl * 4 + wave; u < units; u += slices * 4) {  // wave-uniform
        const int h = u / nseg, seg = u - h * nseg, col = seg * 256 + lane * 4;
        const bool live = col < W;                            // W % 4 == 0: a vector is inside the row or outside it
        const uint32_t at = (uint32_t)h * W + (live ? col : W - 4);
        const f32x4 x = *(const f32x4*)(p + at), y = *(const f32x4*)(t + at);
        f32x4 mv = y;
        if constexpr (BASE) mv = *(const f32x4*)(bp + at);
        uint32_t ef[K], eo[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ef[k] = eo[k] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool valid = x[e] == x[e] && y[e] == y[e] && (!BASE || mv[e] == mv[e]);
            ninv += live && !valid ? 1 : 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float q = BASE ? mv[e] + th[k] : th[k];
                ef[k] |= (valid && fss_is<BELOW>(x[e], q) ? 1u : 0u) << e;
                eo[k] |= (valid && fss_is<BELOW>(y[e], q) ? 1u : 0u) << e;
            }
        }
        const int shn = 4 * (lane & 7), wi = seg * 8 + (lane >> 3);
        const bool owner = (lane & 7) == 0 && wi < WB;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t vf = fss_or8(live ? ef[k] << shn : 0u), vo = fss_or8(live ? eo[k] << shn : 0u);
            if (owner) {
                out[((size_t)(k * 2 + 0) * H + h) * WB + wi] = vf;
                out[((size_t)(k * 2 + 1) * H + h) * WB + wi] = vo;
            }
        }
    }
    __shared__ int ri[4];
    ninv = plane_wave_sum(ninv);
    if (lane == 0) ri[wave] = ninv;
    __syncthreads();
    if (threadIdx.x == 0) inv[pl * slices + sl] = plane_block_total(ri);
}

__global__ __launch_bounds__(256) void fss_box_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ inv, fss_scales sc, int S, int K, int H,
                                                      int W, int band, int nbands, int rmax, int slices, long long* __restrict__ rows,
                                                      int* __restrict__ n_invalid) {
    extern __shared__ unsigned long long fss_lds[];
    const int tid = threadIdx.x;
    const int bd = blockIdx.x % nbands, pk = blockIdx.x / nbands;      // pk = plane * K + k
    const int h0 = bd * band, h1 = min(H, h0 + band), nrows = band + 2 * rmax;
    const int WB = fss_words(W), ntiles = fss_tiles(W), tcols = fss_tile_cols(W), stride = fss_image_stride(W);
    unsigned long long* acc = fss_lds;                        // [h1 - h0][S][3]
    uint32_t* img = (uint32_t*)(fss_lds + (size_t)band * S * 3);       // [2][nrows][stride]
    if (bd == 0 && pk % K == 0) {                             // workgroup-uniform: this plane's invalid points
        __shared__ int ri[4];
        const int plane = pk / K;
        int n = 0;
        for (int i = tid; i < slices; i += 256) n += inv[(size_t)plane * slices + i];
        n = plane_wave_sum(n);
        if ((tid & 63) == 0) ri[tid >> 6] = n;
        __syncthreads();
        if (tid == 0) n_invalid[plane] = plane_block_total(ri);
    }
    for (int i = tid; i < (h1 - h0) * S * 3; i += 256) acc[i] = 0ull;
    const uint32_t* gbits = bits + (size_t)pk * 2 * H * WB;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int c0 = tile * tcols, tc = min(W, c0 + tcols) - c0;
        if (tile) __syncthreads();                            // the walk of the previous tile has read its image
        for (int i = tid; i < 2 * nrows * stride; i += 256) {
            const int f = i / (nrows * stride), rem = i - f * nrows * stride, ir = rem / stride, iw = rem - ir * stride;
            img[i] = fss_image_word(gbits + (size_t)f * H * WB, H, W, h0, rmax, c0, ir, iw);
        }
        __syncthreads();                                      // (also: the accumulators are zero)
        const int nj = (tc + 255) >> 8;                         // 1 .. FSS_CPT, workgroup-uniform
        for (int si = 0; si < S; ++si) {
            const int r = sc.r[si];
            auto emit = [&](int row, uint32_t d2, uint32_t f2, uint32_t o2) {
                d2 = fss_sum16(d2), f2 = fss_sum16(f2), o2 = fss_sum16(o2);        // 16 * 4 * 4225^2 < 2^32
                if ((tid & 15) == 0) {
                    unsigned long long* a = acc + ((size_t)row * S + si) * 3;
                    atomicAdd(a + 0, (unsigned long long)d2);
                    atomicAdd(a + 1, (unsigned long long)f2);
                    atomicAdd(a + 2, (unsigned long long)o2);
                }
            };
            auto walk = [&](auto NJ, auto WIDE) {
                fss_walk<decltype(NJ)::value, decltype(WIDE)::value>(img, img + nrows * stride, stride, tid, h0, h1, rmax, c0, tc, r, emit);
            };
            auto pick = [&](auto WIDE) {
                using std::integral_constant;
                if (nj == 1) walk(integral_constant<int, 1>{}, WIDE);
                else if (nj == 2) walk(integral_constant<int, 2>{}, WIDE);
                else if (nj == 3) walk(integral_constant<int, 3>{}, WIDE);
                else walk(integral_constant<int, 4>{}, WIDE);
            };
            if (r >= 16) pick(std::true_type{}); else pick(std::false_type{});
        }
    }
    __syncthreads();
    for (int i = tid; i < (h1 - h0) * S * 3; i += 256) {
        const int row = i / (S * 3), rem = i - row * S * 3, si = rem / 3, j = rem - si * 3;
        rows[(((size_t)pk * S + si) * H + h0 + row) * 3 + j] = (long long)acc[i];
    }
}

// The workspace, carved here and nowhere else (offsets in 4-byte words)
struct fss_ws {
    size_t inv_at, words;
    fss_ws(size_t planes, int slices, int K, int H, int W) : inv_at(planes * K * 2 * H * fss_words(W)), words(inv_at + planes * slices) {}
    size_t bytes() const { return words * 4; }
    uint32_t* bits(const void* ws) const { return (uint32_t*)ws; }
    int* inv(const void* ws) const { return (int*)ws + inv_at; }
};

// ---- the ensemble: neighbourhood ensemble probabilities (Schwartz et al. 2010) under the same score (Duc et al. 2013) ----------------------
// With c(h, w) = the number of the M members with the event at the point (0 .. M; an invalid point -- a NaN in ANY member, the truth or
// the base -- is an event in no member and not in the analysis), N_f = the box sum of c and n_o that of the analysis bit:
//     rows[B][C][K][S][H][3] = (sum_w (N_f - M n_o)^2, sum_w N_f^2, sum_w n_o^2)          int64, exact
// The same two launches behind swv2_fss_ens_rows:
//   launch 1  fss_ens_mask_kernel<K, BASE, BELOW>   the units and workgroup index of fss_mask_kernel; the members stream past in batches of
//             FSS_ENS_MBATCH loads issued before their first use (as ens_event_sums_kernel: no member is kept, one kernel for every M).  A
//             lane keeps K registers of four 7-bit counts (one byte per point) and writes c as P = bit_length(M) BIT PLANES, plane p
//             holding bit p of c, plus the analysis bit row: bits[plane][k][P + 1][H][ceil(W / 32)], field P = the analysis.
//   launch 2  fss_ens_box_kernel                    one workgroup per (plane, threshold, band).  The LDS image holds the P + 1 extended bit
//             rows of every image row; a forecast window count is sum_p popcount(window of plane p) << p, every piece of it through
//             fss_window on an image built by fss_image_word, the analysis side is the deterministic one.
// Plan (fss_ens_plan_of, the one statement; swv2_fss_ens_band_rows asks it).  The image is (P + 1) / 2 times the deterministic one and a
// workgroup may take FSS_ENS_LDS_MAX = 80 KiB (two per CU).  A band stays as tall as the largest box (the rule above): where a band of
// that height does not fit at 1024-column tiles the TILE is halved (to 512, then 256 columns) before the band is cut, because a band
// shorter than the box pays its 2 r start-up window counts -- P + 1 popcount chains each -- more often than it walks, while a narrower tile
// only rebuilds 64 + columns of halo per tile, a copy.  The band is then the deterministic rule under the tallest band that fits.
// Integer bounds.  N_f <= 64 * 4225 = 270 400 < 2^19 and M n_o likewise (int).  A square is < 2^37: from here on everything is 64-bit.  A
// thread adds at most 4 of them (< 2^39); the 16 lanes of a DPP row add them as two 32-bit halves, the low 24 bits (16 * 2^24 = 2^28) and
// the rest (16 * 2^15 = 2^19), recombined before the 64-bit integer ds_add (< 2^43); n_o^2 keeps the deterministic 32-bit path.  A row sum at
// W = 16384 is < 2^51.
constexpr int FSS_ENS_MAX_M = 64;
constexpr int FSS_ENS_MBATCH = 8;
constexpr int FSS_ENS_TILE_MIN = 256;
constexpr size_t FSS_ENS_LDS_MAX = 80 * 1024;

__host__ __device__ inline int fss_ens_bit_planes(int M) { return 32 - __builtin_clz((unsigned)M); }          // bit_length(M): 2 .. 7
__host__ __device__ inline size_t fss_ens_lds_bytes(int fields, int tcols, int band, int rmax, int S) {
    return (size_t)band * S * 3 * 8 + (size_t)fields * (band + 2 * rmax) * fss_stride_of(tcols) * 4;
}

// the plan: rows per band and the widest column tile, for the worst case of 8 scales and a grid as wide as the tile
struct fss_ens_plan { int band, tile; };
__host__ __device__ inline fss_ens_plan fss_ens_plan_of(long planes, int H, int M, int K, int rmax) {
    const int fields = fss_ens_bit_planes(M) + 1;
    int tall = fss_tall(rmax) < FSS_BAND_MAX ? fss_tall(rmax) : FSS_BAND_MAX, tile = FSS_TILE_COLS, most = FSS_BAND_MAX;
    while (tile > FSS_ENS_TILE_MIN && fss_ens_lds_bytes(fields, tile, tall, rmax, FSS_MAX_S) > FSS_ENS_LDS_MAX) tile >>= 1;
    while (most > 1 && fss_ens_lds_bytes(fields, tile, most, rmax, FSS_MAX_S) > FSS_ENS_LDS_MAX) --most;      // (256 columns, 8 fields, r = 32: 90 rows fit)
    return {fss_bands(planes * K, H, tall, most), tile};
}

template <int K, bool BASE, bool BELOW>
__global__ __launch_bounds__(256) void fss_ens_mask_kernel(const float* __restrict__ ens, long ens_ms, long ens_bs, const float* __restrict__ tar,
                                                           long tar_bs, const float* __restrict__ base, const float* __restrict__ thr, long thr_bs,
                                                           uint32_t* __restrict__ bits, int* __restrict__ inv, int M, int P, int B, int C, int H, int W,
                                                           int slices) {
    const auto [b, c, sl] = plane_shared_index(B, slices);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int WB = fss_words(W), nseg = (W + 255) >> 8;
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    const float* x0p = ens + b * ens_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    const float* bp = BASE ? base + (long)c * plane : nullptr;
    const size_t pl = (size_t)b * C + c;
    uint32_t* out = bits + pl * K * (P + 1) * H * WB;
    float thk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) thk[k] = thr[b * thr_bs + (long)c * K + k];
    int ninv = 0;
    const int units = H * nseg;                               // <= H W / 4
    for (int u = sl * 4 + wave; u < units; u += slices * 4) {  // wave-uniform
        const int h = u / nseg, seg = u - h * nseg, col = seg * 256 + lane * 4;
        const bool live = col < W;                            // W % 4 == 0: a vector is inside the row or outside it
        const uint32_t ib = ((uint32_t)h * W + (live ? col : W - 4)) * 4;       // the lane's byte offset beside one wave-uniform base per member
        const f32x4 y = *(const f32x4*)((const char*)t + ib);
        f32x4 mv = y;
        if constexpr (BASE) mv = *(const f32x4*)((const char*)bp + ib);
        float th[K][4];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) th[k][e] = BASE ? mv[e] + thk[k] : thk[k];
        uint32_t cnt[K];                                      // byte e: the members with the event at point e, at most 64
#pragma unroll
        for (int k = 0; k < K; ++k) cnt[k] = 0u;
        bool bad[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bad[e] = y[e] != y[e] || (BASE && mv[e] != mv[e]);
        for (int m0 = 0; m0 < M; m0 += FSS_ENS_MBATCH) {
            f32x4 xv[FSS_ENS_MBATCH];
#pragma unroll
            for (int j = 0; j < FSS_ENS_MBATCH; ++j)              // the last batch reads member M - 1 again where it has no member of its own
                xv[j] = *(const f32x4*)((const char*)(x0p + (long)min(m0 + j, M - 1) * ens_ms) + ib);
#pragma unroll
            for (int j = 0; j < FSS_ENS_MBATCH; ++j)
                if (m0 + j < M) {                                 // wave-uniform
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bad[e] = bad[e] || xv[j][e] != xv[j][e];
#pragma unroll
                        for (int k = 0; k < K; ++k) cnt[k] += (fss_is<BELOW>(xv[j][e], th[k][e]) ? 1u : 0u) << (8 * e);
                    }
                }
        }
        uint32_t keep = 0u;                                   // the bytes of the valid points
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            keep |= bad[e] ? 0u : 0xffu << (8 * e);
            ninv += live && bad[e] ? 1 : 0;
        }
        const int shn = 4 * (lane & 7), wi = seg * 8 + (lane >> 3);
        const bool owner = (lane & 7) == 0 && wi < WB;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t ck = cnt[k] & keep;
            uint32_t eo = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) eo |= (!bad[e] && fss_is<BELOW>(y[e], th[k][e]) ? 1u : 0u) << e;
            uint32_t* ok = out + (size_t)k * (P + 1) * H * WB + (size_t)h * WB + wi;
            for (int p = 0; p < P; ++p) {                     // wave-uniform: bit p of the four counts -> a nibble
                const uint32_t q = (ck >> p) & 0x01010101u, nib = (q | q >> 7 | q >> 14 | q >> 21) & 0xfu;
                const uint32_t v = fss_or8(live ? nib << shn : 0u);
                if (owner) ok[(size_t)p * H * WB] = v;
            }
            const uint32_t vo = fss_or8(live ? eo << shn : 0u);
            if (owner) ok[(size_t)P * H * WB] = vo;
        }
    }
    __shared__ int ri[4];
    ninv = plane_wave_sum(ninv);
    if (lane == 0) ri[wave] = ninv;
    __syncthreads();
    if (threadIdx.x == 0) inv[pl * slices + sl] = plane_block_total(ri);
}

// the forecast's window count: the set bits of the 2 r + 1 image bits from bit s on in every bit plane (`fs` words apart), weighted 2^p
// (P is a template argument so that the reads of all planes are in flight together: as a run-time loop the planes were read one LDS
// latency after the other at two waves per SIMD)
template <bool WIDE, int P>
__host__ __device__ inline int fss_ens_window(const uint32_t* row, int fs, int s, const fss_mask3 m) {
    int n = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) n += fss_window<WIDE>(row + (size_t)p * fs, s, m) << p;
    return n;
}

// fss_walk for the ensemble: img = the P + 1 images (`fs` words each, the analysis last); emit(row of the band, d2, f2, o2) with the 64-bit
// shares of sum (N_f - M n_o)^2 and sum N_f^2 (each at most 4 * 270 400^2 < 2^39) and the 32-bit one of sum n_o^2
template <int P, int NJ, bool WIDE, class Emit>
__host__ __device__ inline void fss_ens_walk(const uint32_t* img, int M, int fs, int stride, int tid, int h0, int h1, int rmax, int c0, int tc,
                                             int r, Emit&& emit) {
    const fss_mask3 m = fss_window_masks(r);
    const uint32_t* imgO = img + (size_t)P * fs;
    int s[NJ], nf[NJ], no[NJ];
    bool ok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = c0 + tid + 256 * j;
        ok[j] = c < c0 + tc;
        s[j] = (ok[j] ? c : c0 + tc - 1) + 32 - r - 32 * (c0 >> 5);          // the window's first image bit (a spare thread: the last column's)
        nf[j] = no[j] = 0;
    }
    for (int g = h0 - r; g < h0 + r; ++g) {                   // the box of row h0 without its last row
        const int at = (g - h0 + rmax) * stride;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            nf[j] += fss_ens_window<WIDE, P>(img + at, fs, s[j], m);
            no[j] += fss_window<WIDE>(imgO + at, s[j], m);
        }
    }
    for (int h = h0; h < h1; ++h) {
        const int in = (h + r - h0 + rmax) * stride, out = (h - r - h0 + rmax) * stride;
        unsigned long long d2 = 0, f2 = 0;
        uint32_t o2 = 0;                                      // at most 4 * 4225^2
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            nf[j] += fss_ens_window<WIDE, P>(img + in, fs, s[j], m);
            no[j] += fss_window<WIDE>(imgO + in, s[j], m);
            if (ok[j]) {
                const long long d = nf[j] - M * no[j];          // |d| <= 270 400
                d2 += (unsigned long long)(d * d);
                f2 += (unsigned long long)((long long)nf[j] * nf[j]);
                o2 += (uint32_t)(no[j] * no[j]);
            }
            nf[j] -= fss_ens_window<WIDE, P>(img + out, fs, s[j], m);
            no[j] -= fss_window<WIDE>(imgO + out, s[j], m);
        }
        emit(h - h0, d2, f2, o2);
    }
}

// sum over the 16 lanes of a DPP row of values below 2^39: the low 24 bits and the rest, each in 32 bits (16 * 2^24, 16 * 2^15)
__device__ __forceinline__ unsigned long long fss_sum16_u39(unsigned long long v) {
    const uint32_t lo = fss_sum16((uint32_t)v & 0xffffffu), hi = fss_sum16((uint32_t)(v >> 24));
    return ((unsigned long long)hi << 24) + lo;
}

template <int P>
__global__ __launch_bounds__(256) void fss_ens_box_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ inv, fss_scales sc, int S, int K, int M,
                                                          int H, int W, int band, int nbands, int tile, int rmax, int slices,
                                                          long long* __restrict__ rows, int* __restrict__ n_invalid) {
    extern __shared__ unsigned long long fss_ens_lds[];
    const int tid = threadIdx.x;
    const int bd = blockIdx.x % nbands, pk = blockIdx.x / nbands;      // pk = plane * K + k
    const int h0 = bd * band, h1 = min(H, h0 + band), nrows = band + 2 * rmax;
    const int WB = fss_words(W), ntiles = fss_tiles(W, tile), tcols = fss_tile_cols(W, tile), stride = fss_stride_of(tcols), fs = nrows * stride;
    unsigned long long* acc = fss_ens_lds;                    // [h1 - h0][S][3]
    uint32_t* img = (uint32_t*)(fss_ens_lds + (size_t)band * S * 3);   // [P + 1][nrows][stride]
    if (bd == 0 && pk % K == 0) {                             // workgroup-uniform: this plane's invalid points
        __shared__ int ri[4];
        const int plane = pk / K;
        int n = 0;
        for (int i = tid; i < slices; i += 256) n += inv[(size_t)plane * slices + i];
        n = plane_wave_sum(n);
        if ((tid & 63) == 0) ri[tid >> 6] = n;
        __syncthreads();
        if (tid == 0) n_invalid[plane] = plane_block_total(ri);
    }
    for (int i = tid; i < (h1 - h0) * S * 3; i += 256) acc[i] = 0ull;
    const uint32_t* gbits = bits + (size_t)pk * (P + 1) * H * WB;
    for (int tl = 0; tl < ntiles; ++tl) {
        const int c0 = tl * tcols, tc = min(W, c0 + tcols) - c0;
        if (tl) __syncthreads();                              // the walk of the previous tile has read its image
        for (int i = tid; i < (P + 1) * fs; i += 256) {
            const int f = i / fs, rem = i - f * fs, ir = rem / stride, iw = rem - ir * stride;
            img[i] = fss_image_word(gbits + (size_t)f * H * WB, H, W, h0, rmax, c0, ir, iw);
        }
        __syncthreads();                                      // (also: the accumulators are zero)
        const int nj = (tc + 255) >> 8;                         // 1 .. FSS_CPT, workgroup-uniform
        for (int si = 0; si < S; ++si) {
            const int r = sc.r[si];
            auto emit = [&](int row, unsigned long long d2, unsigned long long f2, uint32_t o2) {
                d2 = fss_sum16_u39(d2), f2 = fss_sum16_u39(f2), o2 = fss_sum16(o2);
                if ((tid & 15) == 0) {
                    unsigned long long* a = acc + ((size_t)row * S + si) * 3;
                    atomicAdd(a + 0, d2);
                    atomicAdd(a + 1, f2);
                    atomicAdd(a + 2, (unsigned long long)o2);
                }
            };
            auto walk = [&](auto NJ, auto WIDE) {
                fss_ens_walk<P, decltype(NJ)::value, decltype(WIDE)::value>(img, M, fs, stride, tid, h0, h1, rmax, c0, tc, r, emit);
            };
            auto pick = [&](auto WIDE) {
                using std::integral_constant;
                if (nj == 1) walk(integral_constant<int, 1>{}, WIDE);
                else if (nj == 2) walk(integral_constant<int, 2>{}, WIDE);
                else if (nj == 3) walk(integral_constant<int, 3>{}, WIDE);
                else walk(integral_constant<int, 4>{}, WIDE);
            };
            if (r >= 16) pick(std::true_type{}); else pick(std::false_type{});
        }
    }
    __syncthreads();
    for (int i = tid; i < (h1 - h0) * S * 3; i += 256) {
        const int row = i / (S * 3), rem = i - row * S * 3, si = rem / 3, j = rem - si * 3;
        rows[(((size_t)pk * S + si) * H + h0 + row) * 3 + j] = (long long)acc[i];
    }
}

// The ensemble's workspace: uint32_t bits[planes][K][P + 1][H][ceil(W / 32)], int inv[planes][slices]
struct fss_ens_ws {
    size_t inv_at, words;
    fss_ens_ws(size_t planes, int slices, int K, int P, int H, int W) : inv_at(planes * K * (P + 1) * H * fss_words(W)), words(inv_at + planes * slices) {}
    size_t bytes() const { return words * 4; }
    uint32_t* bits(const void* ws) const { return (uint32_t*)ws; }
    int* inv(const void* ws) const { return (int*)ws + inv_at; }
};

}  // namespace

extern "C" int swv2_fss_ens_band_rows(int planes, int H, int M, int K, int r_max) {
    if (planes <= 0 || H <= 0 || M < 2 || M > FSS_ENS_MAX_M || K < 1 || K > FSS_MAX_K || r_max < 0 || r_max > FSS_MAX_R) return 0;
    return fss_ens_plan_of(planes, H, M, K, r_max).band;
}

extern "C" size_t swv2_fss_ens_ws_bytes(int planes, int H, int W, int M, int K, int S) {
    if (planes <= 0 || H <= 0 || W <= 0 || M < 2 || M > FSS_ENS_MAX_M || K < 1 || K > FSS_MAX_K || S < 1 || S > FSS_MAX_S) return 0;
    return fss_ens_ws((size_t)planes, plane_slices(planes), K, fss_ens_bit_planes(M), H, W).bytes();
}

extern "C" int swv2_fss_ens_rows(const float* ens, long ens_mstride, long ens_bstride, const float* tar, long tar_bstride, const float* base,
                                 const float* thr, long thr_bstride, const int* scales, int M, int K, int S, int below, int B, int C, int H, int W,
                                 void* ws, size_t ws_bytes, long long* rows, int* n_invalid, void* stream) {
    SWV2_CHECK_ARG(ens && tar && thr && scales && ws && rows && n_invalid, "swv2_fss_ens_rows: null pointer");
    SWV2_CHECK_ARG(M >= 2 && M <= FSS_ENS_MAX_M, "swv2_fss_ens_rows: members M outside 2 .. 64");
    SWV2_CHECK_ARG(K >= 1 && K <= FSS_MAX_K, "swv2_fss_ens_rows: thresholds K outside 1 .. 8");
    SWV2_CHECK_ARG(S >= 1 && S <= FSS_MAX_S, "swv2_fss_ens_rows: scales S outside 1 .. 8");
    SWV2_CHECK_ARG(W > 0 && W % 4 == 0, "swv2_fss_ens_rows: W %% 4 != 0");
    SWV2_CHECK_ARG(ens_mstride % 4 == 0, "swv2_fss_ens_rows: member stride not a multiple of 4");
    fss_scales sc{};
    for (int i = 0; i < S; ++i) {
        SWV2_CHECK_ARG(scales[i] >= 0 && scales[i] <= FSS_MAX_R, "swv2_fss_ens_rows: scale %d = %d outside 0 .. 32", i, scales[i]);
        SWV2_CHECK_ARG(i == 0 || scales[i] > scales[i - 1], "swv2_fss_ens_rows: scales not strictly ascending");
        SWV2_CHECK_ARG(2 * scales[i] + 1 <= W, "swv2_fss_ens_rows: scale %d: the box of 2 * %d + 1 columns is wider than W = %d", i, scales[i], W);
        sc.r[i] = scales[i];
    }
    SWV2_CHECK_ARG(((uintptr_t)thr & 3) == 0 && (thr_bstride == 0 || B == 1 || thr_bstride >= (long)C * K),
                   "swv2_fss_ens_rows: thresholds not 4-byte aligned, or a batch stride that is neither 0 nor at least C * K");
    SWV2_CHECK_ARG(((uintptr_t)rows & 7) == 0 && ((uintptr_t)n_invalid & 3) == 0, "swv2_fss_ens_rows: rows not 8-byte aligned or n_invalid not 4-byte aligned");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "swv2_fss_ens_rows: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("swv2_fss_ens_rows", {ens, tar, base, ws}, {ens_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes,
                           swv2_fss_ens_ws_bytes(B * C, H, W, M, K, S), "swv2_fss_ens_ws_bytes"))
        return SWV2_ERR_INVALID;
    const long planes = (long)B * C;
    const int slices = plane_slices(planes), rmax = sc.r[S - 1], P = fss_ens_bit_planes(M);
    const fss_ens_plan plan = fss_ens_plan_of(planes, H, M, K, rmax);
    const int nbands = (H + plan.band - 1) / plan.band;
    SWV2_CHECK_ARG(planes * K * nbands < (1L << 31), "swv2_fss_ens_rows: too many (plane, threshold, band) workgroups");
    const fss_ens_ws lay((size_t)planes, slices, K, P, H, W);
    uint32_t* bits = lay.bits(ws);
    int* inv = lay.inv(ws);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid_a((unsigned)(planes * slices));
#define FSS_LAUNCH(KK)                                                                                                                       \
    do {                                                                                                                                     \
        auto go = [&](auto kern) {                                                                                                           \
            hipLaunchKernelGGL(kern, grid_a, dim3(256), 0, st, ens, ens_mstride, ens_bstride, tar, tar_bstride, base, thr, thr_bstride, bits, inv, M, P, \
                               B, C, H, W, slices);                                                                                          \
        };                                                                                                                                   \
        if (base) { if (below) go(fss_ens_mask_kernel<KK, true, true>); else go(fss_ens_mask_kernel<KK, true, false>); }                     \
        else      { if (below) go(fss_ens_mask_kernel<KK, false, true>); else go(fss_ens_mask_kernel<KK, false, false>); }                   \
    } while (0)
    switch (K) {
        case 1: FSS_LAUNCH(1); break; case 2: FSS_LAUNCH(2); break; case 3: FSS_LAUNCH(3); break; case 4: FSS_LAUNCH(4); break;
        case 5: FSS_LAUNCH(5); break; case 6: FSS_LAUNCH(6); break; case 7: FSS_LAUNCH(7); break; case 8: FSS_LAUNCH(8); break;
    }
#undef FSS_LAUNCH
    SWV2_CHECK_LAUNCH("swv2_fss_ens_rows (masks)");
    auto boxes = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)(planes * K * nbands)), dim3(256), fss_ens_lds_bytes(P + 1, fss_tile_cols(W, plan.tile), plan.band, rmax, S),
                           st, (const uint32_t*)bits, (const int*)inv, sc, S, K, M, H, W, plan.band, nbands, plan.tile, rmax, slices, rows, n_invalid);
    };
    switch (P) {                                              // bit_length(M), M = 2 .. 64
        case 2: boxes(fss_ens_box_kernel<2>); break; case 3: boxes(fss_ens_box_kernel<3>); break; case 4: boxes(fss_ens_box_kernel<4>); break;
        case 5: boxes(fss_ens_box_kernel<5>); break; case 6: boxes(fss_ens_box_kernel<6>); break; case 7: boxes(fss_ens_box_kernel<7>); break;
    }
    SWV2_CHECK_LAUNCH("swv2_fss_ens_rows (boxes)");
    return SWV2_OK;
}

extern "C" int swv2_fss_band_rows(int planes, int H, int K, int r_max) {
    if (planes <= 0 || H <= 0 || K < 1 || K > FSS_MAX_K || r_max < 0 || r_max > FSS_MAX_R) return 0;
    return fss_band_rows(planes, H, K, r_max);
}

extern "C" size_t swv2_fss_ws_bytes(int planes, int H, int W, int K, int S) {
    if (planes <= 0 || H <= 0 || W <= 0 || K < 1 || K > FSS_MAX_K || S < 1 || S > FSS_MAX_S) return 0;
    return fss_ws((size_t)planes, plane_slices(planes), K, H, W).bytes();
}

extern "C" int swv2_fss_rows(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* base, const float* thr,
                             long thr_bstride, const int* scales, int K, int S, int below, int B, int C, int H, int W, void* ws, size_t ws_bytes,
                             long long* rows, int* n_invalid, void* stream) {
    SWV2_CHECK_ARG(prd && tar && thr && scales && ws && rows && n_invalid, "swv2_fss_rows: null pointer");
    SWV2_CHECK_ARG(K >= 1 && K <= FSS_MAX_K, "swv2_fss_rows: thresholds K outside 1 .. 8");
    SWV2_CHECK_ARG(S >= 1 && S <= FSS_MAX_S, "swv2_fss_rows: scales S outside 1 .. 8");
    SWV2_CHECK_ARG(W > 0 && W % 4 == 0, "swv2_fss_rows: W %% 4 != 0");
    fss_scales sc{};
    for (int i = 0; i < S; ++i) {
        SWV2_CHECK_ARG(scales[i] >= 0 && scales[i] <= FSS_MAX_R, "swv2_fss_rows: scale %d = %d outside 0 .. 32", i, scales[i]);
        SWV2_CHECK_ARG(i == 0 || scales[i] > scales[i - 1], "swv2_fss_rows: scales not strictly ascending");
        SWV2_CHECK_ARG(2 * scales[i] + 1 <= W, "swv2_fss_rows: scale %d: the box of 2 * %d + 1 columns is wider than W = %d", i, scales[i], W);
        sc.r[i] = scales[i];
    }
    SWV2_CHECK_ARG(((uintptr_t)thr & 3) == 0 && (thr_bstride == 0 || B == 1 || thr_bstride >= (long)C * K),
                   "swv2_fss_rows: thresholds not 4-byte aligned, or a batch stride that is neither 0 nor at least C * K");
    SWV2_CHECK_ARG(((uintptr_t)rows & 7) == 0 && ((uintptr_t)n_invalid & 3) == 0, "swv2_fss_rows: rows not 8-byte aligned or n_invalid not 4-byte aligned");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "swv2_fss_rows: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("swv2_fss_rows", {prd, tar, base, ws}, {prd_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes,
                           swv2_fss_ws_bytes(B * C, H, W, K, S), "swv2_fss_ws_bytes"))
        return SWV2_ERR_INVALID;
    const long planes = (long)B * C;
    const int slices = plane_slices(planes), rmax = sc.r[S - 1];
    const int band = fss_band_rows(planes, H, K, rmax), nbands = (H + band - 1) / band;
    SWV2_CHECK_ARG(planes * K * nbands < (1L << 31), "swv2_fss_rows: too many (plane, threshold, band) workgroups");
    const fss_ws lay((size_t)planes, slices, K, H, W);
    uint32_t* bits = lay.bits(ws);
    int* inv = lay.inv(ws);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid_a((unsigned)(planes * slices));
#define FSS_LAUNCH(KK)                                                                                                                       \
    do {                                                                                                                                     \
        auto go = [&](auto kern) {                                                                                                           \
            hipLaunchKernelGGL(kern, grid_a, dim3(256), 0, st, prd, prd_bstride, tar, tar_bstride, base, thr, thr_bstride, bits, inv, B, C, H, W, slices); \
        };                                                                                                                                   \
        if (base) { if (below) go(fss_mask_kernel<KK, true, true>); else go(fss_mask_kernel<KK, true, false>); }                             \
        else      { if (below) go(fss_mask_kernel<KK, false, true>); else go(fss_mask_kernel<KK, false, false>); }                           \
    } while (0)
    switch (K) {
        case 1: FSS_LAUNCH(1); break; case 2: FSS_LAUNCH(2); break; case 3: FSS_LAUNCH(3); break; case 4: FSS_LAUNCH(4); break;
        case 5: FSS_LAUNCH(5); break; case 6: FSS_LAUNCH(6); break; case 7: FSS_LAUNCH(7); break; case 8: FSS_LAUNCH(8); break;
    }
#undef FSS_LAUNCH
    SWV2_CHECK_LAUNCH("swv2_fss_rows (masks)");
    hipLaunchKernelGGL(fss_box_kernel, dim3((unsigned)(planes * K * nbands)), dim3(256), fss_lds_bytes(W, band, rmax, S), st, (const uint32_t*)bits,
                       (const int*)inv, sc, S, K, H, W, band, nbands, rmax, slices, rows, n_invalid);
    SWV2_CHECK_LAUNCH("swv2_fss_rows (boxes)");
    return SWV2_OK;
}
