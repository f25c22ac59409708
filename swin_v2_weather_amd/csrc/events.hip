// Forecast events: the 2 x 2 contingency table of a deterministic forecast and the Brier sums / reliability counts of an ensemble, for up
// to 8 thresholds at once, per (sample, channel) plane.  One streaming pass each: prediction (or the M members), truth and -- for
// thresholds relative to a base field -- the base are read from HBM exactly once, whatever K is.
//
//   launch 1  event_sums_kernel<K, BASE, BELOW>       8 (12 with a base) B / element    per (plane, slice): 4 K float sums + 1 count -> workspace
//             ens_event_sums_kernel<K, BASE, BELOW>   4 (M + 1) (+ 4) B / element       per (plane, slice): 3 K + 1 float sums, 1 + 2 K (M + 1) counts
//   launch 2  event_finalize_kernel<K> / ens_event_finalize_kernel<K>   one workgroup per channel: folds the slices
//
// Definitions (include/swv2.h states them in full).  theta = thr[b][c][k], or fl32(base[c][h][w] + thr[b][c][k]) with a base field; the
// event is x > theta (x < theta if BELOW), strictly, in fp32; a point is valid if none of its inputs is NaN.  With q = w[row] at a valid
// point and 0 at an invalid one:
//     deterministic   a += q [P and O]   b += q [P and not O]   c += q [not P and O]   d += q [not P and not O]     (four sums of their own)
//     ensemble        n = #{m : x_m event},  o = [truth event]:   S_e += q (n - M o)^2    S_f += q n (M - n)    S_o += q o    W_v += q
//                     cnt[k][o][n] += 1 at valid points
// q is 0 or w[row], never a product, and (n - M o)^2, n (M - n) are integers below 2^12 formed in integer arithmetic: a table cell
// carries the roundings of its additions only (none at all for unit weights and H W <= 2^24), S_e and S_f those plus the one of the fma.
//
// The dominant bin.  For a rare event nearly every point has n = 0, o = 0, and the 64 lanes of a wave would queue up on one LDS counter
// for every (point, threshold).  That bin is never counted: a point in it issues no LDS operation at all, and launch 2 forms
//     cnt[k][0][0] = (H W - n_invalid) - (the sum of the 2 (M + 1) - 1 other counts)
// in integer arithmetic, which is exact.  Every other bin is one integer ds_add per (point, threshold), as the rank histogram of ensemble.hip.
//
// Members stream: a thread keeps K counters per grid point (4 grid points: one 16-byte vector per member) and loads the members in
// batches of EVT_MBATCH, all loads of a batch issued before the first use; no member is kept, so one kernel serves every M (2 .. 64).
//
// Plan and sums: plane_stream.h, with the workgroup index (c * slices + sl) * B + b (the base field is the shared operand) and
// 4 ceil(v / 256) additions in the thread's own running sum, v = 16-byte vectors of the largest slice (tests/event_reference.py::
// chain_length).  A slice without elements stores zeros.  Nothing is zeroed beforehand and there are no float atomics.
//
// Workspace   deterministic: float part[slots][K][4], int inv[slots]                                 slots = planes * slices
//             ensemble:      float part[slots][K][4] = (S_e, S_f, S_o, W_v), int inv[slots], int cnt[slots][K][2][M + 1]
#include "plane_stream.h"

namespace {

constexpr int EVT_MAX_K = 8;
constexpr int EVT_MAX_M = 64;
constexpr int EVT_MBATCH = 8;

template <bool BELOW>
__device__ __forceinline__ bool evt_is(float x, float th) { return BELOW ? x < th : x > th; }

// one 16-byte vector position of the deterministic table: a[4 k + (0 .. 3)] = the cells a, b, c, d of threshold k
template <int K, bool BASE, bool BELOW>
__device__ __forceinline__ void evt_vec(const f32x4 x, const f32x4 y, const f32x4 m, const float q, const float (&thr)[K], float (&a)[4 * K], int& ninv) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool valid = x[e] == x[e] && y[e] == y[e] && (!BASE || m[e] == m[e]);
        const float qv = valid ? q : 0.f;
        ninv += valid ? 0 : 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float th = BASE ? m[e] + thr[k] : thr[k];
            const bool P = evt_is<BELOW>(x[e], th), O = evt_is<BELOW>(y[e], th);
            const float qp = P ? qv : 0.f, qn = P ? 0.f : qv;
            a[4 * k + 0] += O ? qp : 0.f;
            a[4 * k + 1] += O ? 0.f : qp;
            a[4 * k + 2] += O ? qn : 0.f;
            a[4 * k + 3] += O ? 0.f : qn;
        }
    }
}

template <int K, bool BASE, bool BELOW>
__global__ __launch_bounds__(256) void event_sums_kernel(const float* __restrict__ prd, long prd_bs, const float* __restrict__ tar, long tar_bs,
                                                         const float* __restrict__ base, const float* __restrict__ thr, long thr_bs,
                                                         const float* __restrict__ w, float* __restrict__ part, int* __restrict__ inv, int B, int C,
                                                         int H, int W, int slices) {
    const auto [b, c, sl] = plane_shared_index(B, slices);
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* p = prd + b * prd_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    float th[K];
#pragma unroll
    for (int k = 0; k < K; ++k) th[k] = thr[b * thr_bs + (long)c * K + k];
    float s[4 * K];
    int ninv = 0;
    if constexpr (BASE) {
        const float* const op[3] = {p, t, base + (long)c * plane};
        plane_stream_slice(op, lo, hi, W, w, s,
                           [&](const f32x4(&v)[3], float q, float(&a)[4 * K]) { evt_vec<K, true, BELOW>(v[0], v[1], v[2], q, th, a, ninv); });
    } else {
        const float* const op[2] = {p, t};
        plane_stream_slice(op, lo, hi, W, w, s,
                           [&](const f32x4(&v)[2], float q, float(&a)[4 * K]) { evt_vec<K, false, BELOW>(v[0], v[1], v[1], q, th, a, ninv); });      // (m is not read)
    }
    __shared__ float r[4 * K][4];
    __shared__ int ri[4];
    ninv = plane_wave_sum(ninv);
    if ((threadIdx.x & 63) == 0) ri[threadIdx.x >> 6] = ninv;
    plane_block_stage(s, r);
    if (threadIdx.x == 0) {
        const size_t slot = (size_t)(b * C + c) * slices + sl;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = plane_block_total(r[4 * k + j]);
            *(f32x4*)(part + (slot * K + k) * 4) = o;
        }
        inv[slot] = plane_block_total(ri);
    }
}

// One workgroup per channel: wave v folds the slice partials of the planes b = v, v + 4, ... (plane_fold_slices) and lane 0 writes them.
template <int K>
__global__ __launch_bounds__(256) void event_finalize_kernel(const float* __restrict__ part, const int* __restrict__ inv, int slices, int B, int C,
                                                             float* __restrict__ table, int* __restrict__ n_invalid) {
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < B; b += 4) {
        const size_t pl = (size_t)b * C + c;
        f32x4 a[K];
        plane_fold_slices<K>((const f32x4*)part, pl, slices, lane, a);
        int ni;
        plane_fold_slices<1>(inv, pl, slices, lane, &ni);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) *(f32x4*)(table + (pl * K + k) * 4) = a[k];
            n_invalid[pl] = ni;
        }
    }
}

// Ensemble.  A thread's state per vector position: K x 4 integer counters, the truth (and base) vector, one batch of member vectors.
template <int K, bool BASE, bool BELOW>
__global__ __launch_bounds__(256) void ens_event_sums_kernel(const float* __restrict__ ens, long ens_ms, long ens_bs, const float* __restrict__ tar,
                                                             long tar_bs, const float* __restrict__ base, const float* __restrict__ thr, long thr_bs,
                                                             const float* __restrict__ w, float* __restrict__ part, int* __restrict__ inv,
                                                             int* __restrict__ cnt, int M, int B, int C, int H, int W, int slices) {
    const auto [b, c, sl] = plane_shared_index(B, slices);
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* x0p = ens + b * ens_bs + (long)c * plane;
    const float* t = tar + b * tar_bs + (long)c * plane;
    const float* bp = BASE ? base + (long)c * plane : nullptr;
    const int M1 = M + 1, nbins = K * 2 * M1;
    __shared__ int hist[EVT_MAX_K * 2 * (EVT_MAX_M + 1)];
    __shared__ float r[3 * K + 1][4];
    __shared__ int ri[4];
    for (int i = threadIdx.x; i < nbins; i += 256) hist[i] = 0;
    __syncthreads();
    float thk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) thk[k] = thr[b * thr_bs + (long)c * K + k];
    float s[3 * K + 1];
#pragma unroll
    for (int k = 0; k < 3 * K + 1; ++k) s[k] = 0.f;
    int ninv = 0;
    // lo, hi and the slice length are multiples of 4: a vector never straddles hi or a latitude row (W % 4 == 0)
    for (uint32_t i = lo + threadIdx.x * 4; i < hi; i += 1024) {
        const uint32_t ib = i * 4;                            // the lane's 32-bit byte offset beside one wave-uniform base per member
        const f32x4 yv = *(const f32x4*)((const char*)t + ib);
        f32x4 mv = yv;
        if constexpr (BASE) mv = *(const f32x4*)((const char*)bp + ib);
        const float q = w[i / (uint32_t)W];
        float th[K][4];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) th[k][e] = BASE ? mv[e] + thk[k] : thk[k];
        int n[K][4];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) n[k][e] = 0;
        bool bad[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bad[e] = yv[e] != yv[e] || (BASE && mv[e] != mv[e]);
        for (int m0 = 0; m0 < M; m0 += EVT_MBATCH) {
            f32x4 xv[EVT_MBATCH];
#pragma unroll
            for (int u = 0; u < EVT_MBATCH; ++u)                  // the last batch reads member M - 1 again where it has no member of its own
                xv[u] = *(const f32x4*)((const char*)(x0p + (long)min(m0 + u, M - 1) * ens_ms) + ib);
#pragma unroll
            for (int u = 0; u < EVT_MBATCH; ++u)
                if (m0 + u < M) {                                 // wave-uniform
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bad[e] = bad[e] || xv[u][e] != xv[u][e];
#pragma unroll
                        for (int k = 0; k < K; ++k) n[k][e] += evt_is<BELOW>(xv[u][e], th[k][e]) ? 1 : 0;
                    }
                }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float qv = bad[e] ? 0.f : q;
            ninv += bad[e] ? 1 : 0;
            s[3 * K] += qv;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool O = evt_is<BELOW>(yv[e], th[k][e]);
                const int nn = n[k][e], d = nn - (O ? M : 0);
                s[3 * k + 0] = fmaf(qv, (float)(d * d), s[3 * k + 0]);
                s[3 * k + 1] = fmaf(qv, (float)(nn * (M - nn)), s[3 * k + 1]);
                s[3 * k + 2] += O ? qv : 0.f;
                if (!bad[e] && (nn != 0 || O)) atomicAdd(&hist[(k * 2 + (O ? 1 : 0)) * M1 + nn], 1);      // LDS, integer; the bin (0, 0) is derived in launch 2
            }
        }
    }
    ninv = plane_wave_sum(ninv);
    if ((threadIdx.x & 63) == 0) ri[threadIdx.x >> 6] = ninv;
    plane_block_stage(s, r);                                  // after its barrier the wave sums and every count of this workgroup are in LDS
    const size_t slot = (size_t)(b * C + c) * slices + sl;
    if (threadIdx.x == 0) {
        const float wv = plane_block_total(r[3 * K]);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = plane_block_total(r[3 * k + j]);
            o[3] = wv;
            *(f32x4*)(part + (slot * K + k) * 4) = o;
        }
        inv[slot] = plane_block_total(ri);
    }
    for (int i = threadIdx.x; i < nbins; i += 256) cnt[slot * (size_t)nbins + i] = hist[i];
}

// One workgroup per channel.  Floats: wave v folds the planes b = v, v + 4, ... by plane_fold_slices.  Counts: all 256 threads, one
// (b, k, o, n) each per turn, add the slices (integers: any order gives the same); then, per (b, k), the bin (0, 0) from the others and
// hist[0][j] = cnt[0][j] + cnt[1][j] (the workspace keeps o = 0 and o = 1 apart, one LDS add per point; the output's row 0 is their sum).
template <int K>
__global__ __launch_bounds__(256) void ens_event_finalize_kernel(const float* __restrict__ part, const int* __restrict__ inv, const int* __restrict__ cnt,
                                                                 int slices, int M, int B, int C, int npix, float* __restrict__ sums,
                                                                 float* __restrict__ wv, int* hist, int* n_invalid) {
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    const int M1 = M + 1, nbins = K * 2 * M1;
    for (int b = threadIdx.x >> 6; b < B; b += 4) {
        const size_t pl = (size_t)b * C + c;
        f32x4 a[K];
        plane_fold_slices<K>((const f32x4*)part, pl, slices, lane, a);
        int ni;
        plane_fold_slices<1>(inv, pl, slices, lane, &ni);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) sums[(pl * K + k) * 3 + j] = a[k][j];
            wv[pl] = a[0][3];
            n_invalid[pl] = ni;
        }
    }
    for (int e = threadIdx.x; e < B * nbins; e += 256) {
        const int b = e / nbins, i = e - b * nbins;
        const size_t pl = (size_t)b * C + c;
        int n = 0;
        for (int sl = 0; sl < slices; ++sl) n += cnt[(pl * slices + sl) * (size_t)nbins + i];
        hist[pl * nbins + i] = n;
    }
    __syncthreads();                                          // the counts and n_invalid above are this workgroup's own global stores
    for (int e = threadIdx.x; e < B * K; e += 256) {
        const int b = e / K, k = e - b * K;
        const size_t pl = (size_t)b * C + c;
        int* h = hist + pl * nbins + (size_t)k * 2 * M1;
        int others = 0;
        for (int i = 1; i < 2 * M1; ++i) others += h[i];
        h[0] = npix - n_invalid[pl] - others;                 // cnt[k][0][0], the bin nobody counted
        for (int j = 0; j < M1; ++j) h[j] += h[M1 + j];       // row 0 of the output counts the forecasts of n = j whatever was observed
    }
}

// The workspace, carved here and nowhere else (offsets in 4-byte words): float part[slots][K][4], int inv[slots] and -- for the ensemble,
// M > 0 -- int cnt[slots][K][2][M + 1].  The *_sums and *_finalize entry points and the *_ws_bytes queries all go through it.
struct evt_ws {
    size_t inv_at, cnt_at, words;
    evt_ws(size_t slots, int K, int M) : inv_at(slots * K * 4), cnt_at(inv_at + slots), words(cnt_at + (M ? slots * K * 2 * (M + 1) : 0)) {}
    size_t bytes() const { return words * 4; }
    float* part(const void* ws) const { return (float*)ws; }
    int* inv(const void* ws) const { return (int*)ws + inv_at; }
    int* cnt(const void* ws) const { return (int*)ws + cnt_at; }
};

#define EVT_SWITCH_K(K, CALL) \
    switch (K) {              \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; \
    }

}  // namespace

extern "C" size_t swv2_event_ws_bytes(int planes, int H, int W, int K) {
    if (planes <= 0 || H <= 0 || W <= 0 || K < 1 || K > EVT_MAX_K) return 0;
    return evt_ws((size_t)planes * plane_slices(planes), K, 0).bytes();
}

extern "C" size_t swv2_event_ens_ws_bytes(int planes, int H, int W, int M, int K) {
    if (planes <= 0 || H <= 0 || W <= 0 || K < 1 || K > EVT_MAX_K || M < 2 || M > EVT_MAX_M) return 0;
    return evt_ws((size_t)planes * plane_slices(planes), K, M).bytes();
}

extern "C" int swv2_event_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* base, const float* thr,
                               long thr_bstride, const float* w, int K, int below, int B, int C, int H, int W, void* ws, size_t ws_bytes,
                               void* stream) {
    SWV2_CHECK_ARG(prd && tar && thr && w && ws, "swv2_event_sums: null pointer");
    SWV2_CHECK_ARG(K >= 1 && K <= EVT_MAX_K, "swv2_event_sums: thresholds K outside 1 .. 8");
    SWV2_CHECK_ARG(W % 4 == 0, "swv2_event_sums: W %% 4 != 0");
    SWV2_CHECK_ARG(((uintptr_t)thr & 3) == 0 && (thr_bstride == 0 || B == 1 || thr_bstride >= (long)C * K),
                   "swv2_event_sums: thresholds not 4-byte aligned, or a batch stride that is neither 0 nor at least C * K");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "swv2_event_sums: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("swv2_event_sums", {prd, tar, base, ws}, {prd_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes,
                           swv2_event_ws_bytes(B * C, H, W, K), "swv2_event_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const size_t slots = (size_t)B * C * slices;
    const dim3 grid((unsigned)slots);
    const evt_ws lay(slots, K, 0);
    float* part = lay.part(ws);
    int* inv = lay.inv(ws);
    hipStream_t st = (hipStream_t)stream;
#define EVT_LAUNCH(KK)                                                                                                                           \
    do {                                                                                                                                         \
        auto go = [&](auto kern) {                                                                                                               \
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, prd, prd_bstride, tar, tar_bstride, base, thr, thr_bstride, w, part, inv, B, C, H, W, slices); \
        };                                                                                                                                       \
        if (base) { if (below) go(event_sums_kernel<KK, true, true>); else go(event_sums_kernel<KK, true, false>); }                             \
        else      { if (below) go(event_sums_kernel<KK, false, true>); else go(event_sums_kernel<KK, false, false>); }                           \
    } while (0)
    EVT_SWITCH_K(K, EVT_LAUNCH)
#undef EVT_LAUNCH
    SWV2_CHECK_LAUNCH("swv2_event_sums");
    return SWV2_OK;
}

extern "C" int swv2_event_finalize(const void* ws, size_t ws_bytes, int K, int B, int C, int H, int W, float* table, int* n_invalid, void* stream) {
    SWV2_CHECK_ARG(ws && table && n_invalid, "swv2_event_finalize: null pointer");
    SWV2_CHECK_ARG(K >= 1 && K <= EVT_MAX_K, "swv2_event_finalize: thresholds K outside 1 .. 8");
    SWV2_CHECK_ARG(((uintptr_t)n_invalid & 3) == 0, "swv2_event_finalize: n_invalid not 4-byte aligned");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "swv2_event_finalize: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("swv2_event_finalize", {ws, table}, {}, 1, 0, ws_bytes, swv2_event_ws_bytes(B * C, H, W, K), "swv2_event_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const evt_ws lay((size_t)B * C * slices, K, 0);
    const float* part = lay.part(ws);
    const int* inv = lay.inv(ws);
#define EVT_LAUNCH(KK) hipLaunchKernelGGL(event_finalize_kernel<KK>, dim3(C), dim3(256), 0, (hipStream_t)stream, part, inv, slices, B, C, table, n_invalid)
    EVT_SWITCH_K(K, EVT_LAUNCH)
#undef EVT_LAUNCH
    SWV2_CHECK_LAUNCH("swv2_event_finalize");
    return SWV2_OK;
}

extern "C" int swv2_event_ens_sums(const float* ens, long ens_mstride, long ens_bstride, const float* tar, long tar_bstride, const float* base,
                                   const float* thr, long thr_bstride, const float* w, int M, int K, int below, int B, int C, int H, int W,
                                   void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(ens && tar && thr && w && ws, "swv2_event_ens_sums: null pointer");
    SWV2_CHECK_ARG(K >= 1 && K <= EVT_MAX_K, "swv2_event_ens_sums: thresholds K outside 1 .. 8");
    SWV2_CHECK_ARG(M >= 2 && M <= EVT_MAX_M, "swv2_event_ens_sums: members M outside 2 .. 64");
    SWV2_CHECK_ARG(W % 4 == 0, "swv2_event_ens_sums: W %% 4 != 0");
    SWV2_CHECK_ARG(ens_mstride % 4 == 0, "swv2_event_ens_sums: member stride not a multiple of 4");
    SWV2_CHECK_ARG(((uintptr_t)thr & 3) == 0 && (thr_bstride == 0 || B == 1 || thr_bstride >= (long)C * K),
                   "swv2_event_ens_sums: thresholds not 4-byte aligned, or a batch stride that is neither 0 nor at least C * K");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "swv2_event_ens_sums: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("swv2_event_ens_sums", {ens, tar, base, ws}, {ens_bstride, tar_bstride}, B, (long)C * H * W, ws_bytes,
                           swv2_event_ens_ws_bytes(B * C, H, W, M, K), "swv2_event_ens_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const size_t slots = (size_t)B * C * slices;
    const dim3 grid((unsigned)slots);
    const evt_ws lay(slots, K, M);
    float* part = lay.part(ws);
    int* inv = lay.inv(ws);
    int* cnt = lay.cnt(ws);
    hipStream_t st = (hipStream_t)stream;
#define EVT_LAUNCH(KK)                                                                                                                           \
    do {                                                                                                                                         \
        auto go = [&](auto kern) {                                                                                                               \
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, ens, ens_mstride, ens_bstride, tar, tar_bstride, base, thr, thr_bstride, w, part, inv, cnt, M, \
                               B, C, H, W, slices);                                                                                              \
        };                                                                                                                                       \
        if (base) { if (below) go(ens_event_sums_kernel<KK, true, true>); else go(ens_event_sums_kernel<KK, true, false>); }                     \
        else      { if (below) go(ens_event_sums_kernel<KK, false, true>); else go(ens_event_sums_kernel<KK, false, false>); }                   \
    } while (0)
    EVT_SWITCH_K(K, EVT_LAUNCH)
#undef EVT_LAUNCH
    SWV2_CHECK_LAUNCH("swv2_event_ens_sums");
    return SWV2_OK;
}

extern "C" int swv2_event_ens_finalize(const void* ws, size_t ws_bytes, int M, int K, int B, int C, int H, int W, float* sums, float* wv, int* hist,
                                       int* n_invalid, void* stream) {
    SWV2_CHECK_ARG(ws && sums && wv && hist && n_invalid, "swv2_event_ens_finalize: null pointer");
    SWV2_CHECK_ARG(K >= 1 && K <= EVT_MAX_K, "swv2_event_ens_finalize: thresholds K outside 1 .. 8");
    SWV2_CHECK_ARG(M >= 2 && M <= EVT_MAX_M, "swv2_event_ens_finalize: members M outside 2 .. 64");
    SWV2_CHECK_ARG((((uintptr_t)sums | (uintptr_t)wv | (uintptr_t)hist | (uintptr_t)n_invalid) & 3) == 0,
                   "swv2_event_ens_finalize: output pointer not 4-byte aligned");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "swv2_event_ens_finalize: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    if (!plane_operands_ok("swv2_event_ens_finalize", {ws}, {}, 1, 0, ws_bytes, swv2_event_ens_ws_bytes(B * C, H, W, M, K), "swv2_event_ens_ws_bytes"))
        return SWV2_ERR_INVALID;
    const int slices = plane_slices((long)B * C);
    const size_t slots = (size_t)B * C * slices;
    const evt_ws lay(slots, K, M);
    const float* part = lay.part(ws);
    const int* inv = lay.inv(ws);
    const int* cnt = lay.cnt(ws);
#define EVT_LAUNCH(KK)                                                                                                                      \
    hipLaunchKernelGGL(ens_event_finalize_kernel<KK>, dim3(C), dim3(256), 0, (hipStream_t)stream, part, inv, cnt, slices, M, B, C, H * W, sums, wv, hist, \
                       n_invalid)
    EVT_SWITCH_K(K, EVT_LAUNCH)
#undef EVT_LAUNCH
    SWV2_CHECK_LAUNCH("swv2_event_ens_finalize");
    return SWV2_OK;
}
