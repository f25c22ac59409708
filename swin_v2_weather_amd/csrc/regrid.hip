// First-order conservative regridding of [B][C][H][W] planes to [B][C][Hd][Wd] (utils/regrid.py states the operator): y = A x Bm^T with
// banded A [Hd][H] (sin(lat) overlaps) and Bm [Wd][W] (longitude overlaps, periodic), each row given as (start, count, count weights).
//
//     r[J][i] = sum_{k < lat_count[J]} lat_w[J][k] x[lat_start[J] + k][i]                  latitude first: the coalesced direction
//     y[J][I] = sum_{k < lon_count[I]} lon_w[I][k] r[J][(lon_start[I] + k) mod W]          from the row r in LDS
//
// both fp32 fma chains from zero with k ascending.  Entries k >= count are never read: a NaN or Inf of one source cell reaches exactly
// the target cells whose bands contain it.
//
// Work split.  One workgroup of 256 threads per (plane, run of R adjacent target rows), R <= 4.  Phase 1: for each row of the run every
// thread walks down its own 16-byte column vectors (vector v = tid, tid + 256, ...), up to eight row loads issued before the first fma,
// and leaves the W-wide row in LDS (R rows: 23 KB at W = 1440).  One barrier.  Phase 2: the R * Wd outputs of the run are dealt to the
// threads one by one (item = tid, tid + 256, ...); each reads its band from its LDS row and stores one float.  Neighbouring target rows
// share their boundary source row at integer ratios (weights 1/12 each side at 0.25 -> 1.5 degrees): within a run the second read of it
// comes from the cache the first one filled a few hundred cycles earlier, so only the R-th boundary is fetched from memory twice: 1/(6 R)
// of the input at 1.5 degrees, against 1/6 for one row per workgroup.  R is the largest of 4, 2, 1 that the LDS holds and that still
// leaves 1024 workgroups (or 1); an output's two chains do not depend on R.  Every output has one owner: no atomics, nothing pre-zeroed,
// two runs agree bit for bit.
//
// LDS.  Phase 1 writes 16 bytes per lane at consecutive addresses.  Phase 2 reads one dword per lane; neighbouring lanes are W / Wd
// dwords apart (6 at 1440 -> 240: even, so two lanes of a 32-lane half share a bank: 2-way; 22.5 at -> 64: mixed).  The reads are 7 (24)
// per output against 6 (22.5) x 7 (24) bytes-of-four streamed from memory for it, a small share of the LDS pipe either way.
#include "common.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_MAX_RUN = 4;
constexpr int RG_CHUNK = 8;                    // source rows in flight per thread and vector
constexpr int RG_MIN_BLOCKS = 1024;
constexpr long RG_LDS_BYTES = 64 * 1024;

__global__ __launch_bounds__(RG_THREADS) void regrid_kernel(const float* __restrict__ x, long x_bs, float* __restrict__ y, long y_bs, int C, int H,
                                                            int W, int Hd, int Wd, int R, int runs, const int* __restrict__ lat_start,
                                                            const int* __restrict__ lat_count, const float* __restrict__ lat_w, int KH,
                                                            const int* __restrict__ lon_start, const int* __restrict__ lon_count,
                                                            const float* __restrict__ lon_w, int KW) {
    extern __shared__ f32x4 rg_rows[];                                     // [R][W / 4]
    const int pl = blockIdx.x / runs, run = blockIdx.x - pl * runs, b = pl / C, c = pl - b * C;
    const float* const xp = x + b * x_bs + (size_t)c * H * W;
    float* const yp = y + b * y_bs + (size_t)c * Hd * Wd;
    const int J0 = run * R, nr = min(R, Hd - J0), W4 = W >> 2;

    for (int jr = 0; jr < nr; ++jr) {
        const int J = J0 + jr, cnt = lat_count[J];                         // uniform: scalar loads
        const f32x4* const src = (const f32x4*)(xp + (size_t)lat_start[J] * W);
        const float* const wj = lat_w + (size_t)J * KH;
        for (int v = threadIdx.x; v < W4; v += RG_THREADS) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < cnt; k0 += RG_CHUNK) {
                f32x4 t[RG_CHUNK];
#pragma unroll
                for (int u = 0; u < RG_CHUNK; ++u) t[u] = src[(size_t)min(k0 + u, cnt - 1) * W4 + v];        // clamped: unconditional loads
#pragma unroll
                for (int u = 0; u < RG_CHUNK; ++u)
                    if (k0 + u < cnt) {                                    // (uniform) a padded entry is skipped, not multiplied by zero
                        const float wk = wj[k0 + u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = fmaf(wk, t[u][e], acc[e]);
                    }
            }
            rg_rows[jr * W4 + v] = acc;
        }
    }
    __syncthreads();

    const float* const rows = (const float*)rg_rows;
    for (int item = threadIdx.x; item < nr * Wd; item += RG_THREADS) {
        const int jr = item / Wd, I = item - jr * Wd;
        const int st = lon_start[I], cnt = lon_count[I];
        const float* const wi = lon_w + (size_t)I * KW;
        const float* const r = rows + jr * W;
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) {
            int i = st + k;
            i -= i >= W ? W : 0;
            acc = fmaf(wi[k], r[i], acc);
        }
        yp[(size_t)(J0 + jr) * Wd + I] = acc;
    }
}

}  // namespace

extern "C" int swv2_regrid(const float* x, long x_bstride, float* y, long y_bstride, int B, int C, int H, int W, int Hd, int Wd,
                           const int* lat_start, const int* lat_count, const float* lat_w, int KH, const int* lon_start, const int* lon_count,
                           const float* lon_w, int KW, void* stream) {
    SWV2_CHECK_ARG(x && y && lat_start && lat_count && lat_w && lon_start && lon_count && lon_w, "regrid: null pointer");
    SWV2_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && Hd > 0 && Wd > 0, "regrid: bad shape (B, C, H, W, Hd, Wd > 0)");
    SWV2_CHECK_ARG((long)B * C < (1L << 20), "regrid: B * C >= 2^20");
    SWV2_CHECK_ARG((long)H * W < (1L << 30), "regrid: H * W >= 2^30");
    SWV2_CHECK_ARG((long)Hd * Wd < (1L << 30), "regrid: Hd * Wd >= 2^30");
    SWV2_CHECK_ARG(W % 4 == 0, "regrid: W %% 4 != 0");
    SWV2_CHECK_ARG((long)W * 4 <= RG_LDS_BYTES, "regrid: W > 16384 (a source row does not fit the LDS)");
    SWV2_CHECK_ARG(KH >= 1 && KH <= 32 && KW >= 1 && KW <= 32, "regrid: band width outside 1 .. 32");
    SWV2_CHECK_ARG(((uintptr_t)x & 15) == 0, "regrid: x not 16-byte aligned");
    SWV2_CHECK_ARG(x_bstride % 4 == 0 && y_bstride % 4 == 0, "regrid: batch stride not a multiple of 4");
    SWV2_CHECK_ARG(B == 1 || (x_bstride >= (long)C * H * W && y_bstride >= (long)C * Hd * Wd),
                   "regrid: batch stride smaller than the C planes of a sample");
    int R = RG_MAX_RUN;
    while (R > 1 && ((long)R * W * 4 > RG_LDS_BYTES || (long)B * C * cdiv(Hd, R) < RG_MIN_BLOCKS)) R >>= 1;
    const int runs = cdiv(Hd, R);
    SWV2_CHECK_ARG((long)B * C * runs < (1L << 31), "regrid: B * C * Hd too large for the grid index");
    hipLaunchKernelGGL(regrid_kernel, dim3((unsigned)((long)B * C * runs)), dim3(RG_THREADS), (size_t)R * W * sizeof(float), (hipStream_t)stream, x,
                       x_bstride, y, y_bstride, C, H, W, Hd, Wd, R, runs, lat_start, lat_count, lat_w, KH, lon_start, lon_count, lon_w, KW);
    SWV2_CHECK_LAUNCH("swv2_regrid");
    return SWV2_OK;
}
