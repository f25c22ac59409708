// Row-wise (HBM-bound) kernels of the SwinV2 hot path: fused LayerNorm + drop-path + residual (+ window reverse /
// un-roll scatter), its backward, weight preparation, batch sums, fused Adam.
// All of them stream rows with 16-byte accesses; G lanes cooperate on one row (G = 16/32/64 by channel count).
#include "common.h"

namespace {

constexpr int LN_BLOCK = 256;

template <int G>
__device__ __forceinline__ float group_sum(float v) { return group_allsum<G>(v); }       // (vector ALU only: common.h)

// ------------------------------------------------------------------------------------------------
// y[dst] = res[rsrc] + scale[b] * (LN(a[m]) * gamma + beta)
//   a     : [M][C] bf16 branch output (proj or fc2 or patch conv), logical rows m
//   dst   : rowidx ? rowidx[m] : m   (window reverse + un-roll folded into the scatter; <0 = padded row, skipped)
//   res   : fp32 rows; row = res_mod ? dst % res_mod : dst  (res_mod = T broadcasts pos_embed over the batch)
//   scale : per-sample drop-path factor, b = dst / rows_per_sample ; null = 1
// saves mean / rstd per logical row for the backward.  CH = chunks (of 8 channels) per lane.
// reference: x + drop_path(norm(branch(x)))  swinv2_global.py:490,496 ; PatchEmbed norm + pos_embed :545,780
// ------------------------------------------------------------------------------------------------
template <int G, int CH>
__global__ __launch_bounds__(LN_BLOCK) void ln_residual_fwd_kernel(
    const uint16_t* __restrict__ a, const float* __restrict__ res, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ scale, const int32_t* __restrict__ rowidx,
    float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int M, int C, int res_mod,
    int rows_per_sample, float eps) {
    const int gl = threadIdx.x % G;
    const int rows_per_block = LN_BLOCK / G;
    for (long m = (long)blockIdx.x * rows_per_block + threadIdx.x / G; m < M; m += (long)gridDim.x * rows_per_block) {
        long dst = m;
        if (rowidx) dst = rowidx[m];
        float v[CH][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c0 = (gl + i * G) * 8;
            if (c0 < C) {
                unpack8(*(const uint4*)(a + m * C + c0), v[i]);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += v[i][e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
            }
        }
        const float mu = group_sum<G>(s) / C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if ((gl + i * G) * 8 < C) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mu; q = fmaf(d, d, q); }
            }
        const float rs = rsqrtf(group_sum<G>(q) / C + eps);
        if (gl == 0) { mean[m] = mu; rstd[m] = rs; }
        if (dst < 0) continue;
        const float sc = scale ? scale[(int)dst / rows_per_sample] : 1.f;
        const long rrow = res_mod ? (long)((int)dst % res_mod) : dst;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c0 = (gl + i * G) * 8;
            if (c0 >= C) continue;
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const f32x4 gm = *(const f32x4*)(gamma + c0 + 4 * hlf), bt = *(const f32x4*)(beta + c0 + 4 * hlf);
                f32x4 r = res ? *(const f32x4*)(res + rrow * C + c0 + 4 * hlf) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] += sc * ((v[i][4 * hlf + e] - mu) * rs * gm[e] + bt[e]);
                *(f32x4*)(y + dst * C + c0 + 4 * hlf) = r;
            }
        }
    }
}

// backward of the above w.r.t. the branch output a, gamma, beta.  dy is the gradient of y (fp32, destination rows);
// the gradient w.r.t. `res` is dy itself (the caller owns that accumulation).
//   da[m] = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)),  g = scale * dy[dst] * gamma   (zeros for padded rows)
//   dgamma += sum_rows scale * dy * xhat ; dbeta += sum_rows scale * dy      (fp32 atomics, one per column per block)
template <int G, int CH>
__global__ __launch_bounds__(LN_BLOCK) void ln_residual_bwd_kernel(
    const uint16_t* __restrict__ a, const float* __restrict__ dy, const float* __restrict__ gamma,
    const float* __restrict__ scale, const int32_t* __restrict__ rowidx, const float* __restrict__ mean,
    const float* __restrict__ rstd, uint16_t* __restrict__ da, float* __restrict__ ws, int M, int C,
    int rows_per_sample) {
    const int gl = threadIdx.x % G;
    const int rows_per_block = LN_BLOCK / G;
    float dg[CH][8], dbt[CH][8];
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) { dg[i][e] = 0.f; dbt[i][e] = 0.f; }

    for (long m = (long)blockIdx.x * rows_per_block + threadIdx.x / G; m < M; m += (long)gridDim.x * rows_per_block) {
        long dst = m;
        if (rowidx) dst = rowidx[m];
        if (dst < 0) {                               // padded row: zero gradient
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int c0 = (gl + i * G) * 8;
                if (c0 < C) *(uint4*)(da + m * C + c0) = make_uint4(0, 0, 0, 0);
            }
            continue;
        }
        const float mu = mean[m], rs = rstd[m];
        const float sc = scale ? scale[(int)dst / rows_per_sample] : 1.f;
        float xh[CH][8], gg[CH][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c0 = (gl + i * G) * 8;
            if (c0 < C) {
                float av[8];
                unpack8(*(const uint4*)(a + m * C + c0), av);
#pragma unroll
                for (int hlf = 0; hlf < 2; ++hlf) {
                    const f32x4 d4 = *(const f32x4*)(dy + dst * C + c0 + 4 * hlf);
                    const f32x4 gm = *(const f32x4*)(gamma + c0 + 4 * hlf);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = 4 * hlf + e;
                        const float d = sc * d4[e];
                        xh[i][k] = (av[k] - mu) * rs;
                        gg[i][k] = d * gm[e];
                        dg[i][k] = fmaf(d, xh[i][k], dg[i][k]);
                        dbt[i][k] += d;
                        s1 += gg[i][k];
                        s2 = fmaf(gg[i][k], xh[i][k], s2);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) { xh[i][e] = 0.f; gg[i][e] = 0.f; }
            }
        }
        s1 = group_sum<G>(s1) / C;
        s2 = group_sum<G>(s2) / C;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c0 = (gl + i * G) * 8;
            if (c0 >= C) continue;
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = rs * (gg[i][e] - s1 - xh[i][e] * s2);
            *(uint4*)(da + m * C + c0) = pack8(o);
        }
    }
    // block reduction of dgamma / dbeta: rows_per_block partial sums per column
    __shared__ float sg[LN_BLOCK * 8], sb[LN_BLOCK * 8];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c0 = (gl + i * G) * 8;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) { sg[threadIdx.x * 8 + e] = dg[i][e]; sb[threadIdx.x * 8 + e] = dbt[i][e]; }
        __syncthreads();
        if (threadIdx.x < G && c0 < C) {             // first row-group's lanes sum over the row groups
            float tg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int r = 0; r < rows_per_block; ++r)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    tg[e] += sg[(r * G + gl) * 8 + e];
                    tb[e] += sb[(r * G + gl) * 8 + e];
                }
            // per-block partial sums (plain stores); ln_partials_reduce_kernel folds them: thousands of same-address
            // float atomics serialise at the memory side (measured: 7x the kernel's streaming time)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ws[((size_t)blockIdx.x * 2 + 0) * C + c0 + e] = tg[e];
                ws[((size_t)blockIdx.x * 2 + 1) * C + c0 + e] = tb[e];
            }
        }
    }
}

// dgamma[j] += sum_b ws[b][0][j], dbeta[j] += sum_b ws[b][1][j] : 16 columns x 64 slices of blocks per workgroup (a
// launch of 2 C / 16 workgroups; the per-thread chain over ~1000 partial rows is what this tiny kernel's time is, so it is
// spread over 64 slices: 11 -> ~4 us, 25 launches per step)
constexpr int LNR_COLS = 16, LNR_SLICES = 64;
__global__ __launch_bounds__(LNR_COLS * LNR_SLICES) void ln_partials_reduce_kernel(const float* __restrict__ ws,
                                                                                   float* __restrict__ dgamma,
                                                                                   float* __restrict__ dbeta, int nblocks,
                                                                                   int C, const float* __restrict__ ws2,
                                                                                   float* __restrict__ dgamma2,
                                                                                   float* __restrict__ dbeta2, int nblocks2) {
    __shared__ float part[LNR_SLICES][LNR_COLS];
    if (blockIdx.y == 1) { ws = ws2; dgamma = dgamma2; dbeta = dbeta2; nblocks = nblocks2; }      // second set (grid.y = 2)
    const int col = threadIdx.x % LNR_COLS, sl = threadIdx.x / LNR_COLS;
    const int j = blockIdx.x * LNR_COLS + col;
    float s = 0.f;
    if (j < 2 * C) {
#pragma unroll 4
        for (int b = sl; b < nblocks; b += LNR_SLICES) s += ws[(size_t)b * 2 * C + j];
    }
    part[sl][col] = s;
    __syncthreads();
    for (int h = LNR_SLICES / 2; h > 0; h >>= 1) {            // fixed-order tree: deterministic
        if (sl < h) part[sl][col] += part[sl + h][col];
        __syncthreads();
    }
    if (sl == 0 && j < 2 * C) {
        if (j < C) dgamma[j] += part[0][col]; else dbeta[j - C] += part[0][col];
    }
}

// out_bf16[i][j] = W'[rmap ? rmap[i] : i][cmap ? cmap[j] : j]  (0 where a map entry is < 0), W' = transpose ? w^T : w
__global__ void prep_weight_kernel(const float* __restrict__ w, int rows, int cols, int transpose,
                                   const int32_t* __restrict__ rmap, int out_rows, const int32_t* __restrict__ cmap,
                                   int out_cols, uint16_t* __restrict__ out) {
    const long n = (long)out_rows * out_cols;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
        const int i = idx / out_cols, j = idx - (long)i * out_cols;
        const int r = rmap ? rmap[i] : i, c = cmap ? cmap[j] : j;
        float v = 0.f;
        if (r >= 0 && c >= 0) v = transpose ? w[(long)c * cols + r] : w[(long)r * cols + c];
        out[idx] = f2bf(v);
    }
}

// The same for MANY parameters in one launch (every optimizer step changes every weight: ~100 prepared copies for the
// depth-12 model; one workgroup per chunk of PREP_CHUNK output elements, tables in device memory as for adam_multi_kernel).
// out_f32 items keep fp32 (the head-padded qkv bias).
constexpr int PREP_CHUNK = 4096;
// transposed copies of matrices with both dimensions >= 64 are cut into 64 x 64 output tiles instead of linear chunks: the source
// is read along its rows (= down the output's columns) and turned in LDS.  Read element by element in output order every lane
// touches its own line: the embed-768 model's 110 M transposed elements took 2.9 ms per step.
static inline bool prep_tiled(int out_rows, int out_cols, int transpose) { return transpose && out_rows >= 64 && out_cols >= 64; }
__global__ __launch_bounds__(256) void prep_multi_kernel(const swv2_prep_item* __restrict__ items, const int2* __restrict__ chunks) {
    const int2 c = chunks[blockIdx.x];
    const swv2_prep_item it = items[c.x];
    if (it.transpose && it.out_rows >= 64 && it.out_cols >= 64) {
        __shared__ float t[64][65];
        const int tj_n = (it.out_cols + 63) >> 6, i0 = (c.y / tj_n) * 64, j0 = (c.y - (c.y / tj_n) * tj_n) * 64;
        const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
        {
            const int i = i0 + lane, r = i < it.out_rows ? (it.row_map ? it.row_map[i] : i) : -1;       // source column
#pragma unroll 4
            for (int jj = grp; jj < 64; jj += 4) {
                const int j = j0 + jj, cc = j < it.out_cols ? (it.col_map ? it.col_map[j] : j) : -1;   // source row
                t[jj][lane] = (r >= 0 && cc >= 0) ? it.w[(long)cc * it.cols + r] : 0.f;
            }
        }
        __syncthreads();
        const int j = j0 + lane;
        if (j < it.out_cols) {
#pragma unroll 4
            for (int ii = grp; ii < 64; ii += 4) {
                const int i = i0 + ii;
                if (i >= it.out_rows) break;
                const float v = t[lane][ii];
                if (it.out_f32) ((float*)it.out)[(long)i * it.out_cols + j] = v; else ((uint16_t*)it.out)[(long)i * it.out_cols + j] = f2bf(v);
            }
        }
        return;
    }
    const long n = (long)it.out_rows * it.out_cols, lo = (long)c.y * PREP_CHUNK, hi = min(n, lo + PREP_CHUNK);
    for (long idx = lo + threadIdx.x; idx < hi; idx += 256) {
        const int i = idx / it.out_cols, j = idx - (long)i * it.out_cols;
        const int r = it.row_map ? it.row_map[i] : i, cc = it.col_map ? it.col_map[j] : j;
        float v = 0.f;
        if (r >= 0 && cc >= 0) v = it.transpose ? it.w[(long)cc * it.cols + r] : it.w[(long)r * it.cols + cc];
        if (it.out_f32) ((float*)it.out)[idx] = v; else ((uint16_t*)it.out)[idx] = f2bf(v);
    }
}

// out[i] (+)= sum_b in[b][i]
__global__ void batch_sum_kernel(const float* __restrict__ in, float* __restrict__ out, int B, long n, int accumulate) {
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
        f32x4 s = accumulate ? *(const f32x4*)(out + i) : (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < B; ++b) s += *(const f32x4*)(in + (long)b * n + i);
        *(f32x4*)(out + i) = s;
    }
}

// per-row mean / rstd of the 2x2-merged rows (PatchMerging LayerNorm(4C), swinv2_global.py:521)
__global__ void merge_stats_kernel(const float* __restrict__ x, float* __restrict__ mean, float* __restrict__ rstd,
                                   int B, int H, int W, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int h2 = H >> 1, w2 = W >> 1;
    const long M = (long)B * h2 * w2;
    for (long m = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); m < M; m += (long)gridDim.x * (blockDim.x >> 6)) {
        const int b = m / (h2 * w2), ij = m - (long)b * h2 * w2, i = ij / w2, j = ij - i * w2;
        float s = 0.f, q = 0.f;
        for (int k = lane; k < 4 * C; k += 64) {
            const int blk = k / C, c = k - blk * C, wp = blk >> 1, hp = blk & 1;
            const float v = x[(((long)b * H + 2 * i + hp) * W + 2 * j + wp) * C + c];
            s += v;
            q = fmaf(v, v, q);
        }
        s = wave_sum(s);
        q = wave_sum(q);
        const float mu = s / (4 * C);
        const float var = fmaxf(q / (4 * C) - mu * mu, 0.f);
        if (lane == 0) { mean[m] = mu; rstd[m] = rsqrtf(var + eps); }
    }
}

// backward of the PatchMerging LayerNorm + gather: dn [M][4C] bf16 (grad of the normalised rows) -> dx [B][H][W][C]
// fp32 (every x element belongs to exactly one merged row), dgamma / dbeta [4C] via atomics.
__global__ void merge_ln_bwd_kernel(const float* __restrict__ x, const uint16_t* __restrict__ dn,
                                    const float* __restrict__ gamma, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, float* __restrict__ dx, float* __restrict__ dgamma,
                                    float* __restrict__ dbeta, int B, int H, int W, int C) {
    const int lane = threadIdx.x & 63;
    const int h2 = H >> 1, w2 = W >> 1, K = 4 * C;
    const long M = (long)B * h2 * w2;
    for (long m = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); m < M; m += (long)gridDim.x * (blockDim.x >> 6)) {
        const int b = m / (h2 * w2), ij = m - (long)b * h2 * w2, i = ij / w2, j = ij - i * w2;
        const float mu = mean[m], rs = rstd[m];
        float s1 = 0.f, s2 = 0.f;
        for (int k = lane; k < K; k += 64) {
            const int blk = k / C, c = k - blk * C, wp = blk >> 1, hp = blk & 1;
            const float xh = (x[(((long)b * H + 2 * i + hp) * W + 2 * j + wp) * C + c] - mu) * rs;
            const float d = bf2f(dn[m * K + k]);
            const float gg = d * gamma[k];
            s1 += gg;
            s2 = fmaf(gg, xh, s2);
            atomicAdd(dgamma + k, d * xh);
            atomicAdd(dbeta + k, d);
        }
        s1 = wave_sum(s1) / K;
        s2 = wave_sum(s2) / K;
        for (int k = lane; k < K; k += 64) {
            const int blk = k / C, c = k - blk * C, wp = blk >> 1, hp = blk & 1;
            const long xi = (((long)b * H + 2 * i + hp) * W + 2 * j + wp) * C + c;
            const float xh = (x[xi] - mu) * rs;
            const float gg = bf2f(dn[m * K + k]) * gamma[k];
            dx[xi] = rs * (gg - s1 - xh * s2);
        }
    }
}

// fused Adam over one flat fp32 buffer (torch.optim.Adam semantics, train.py:176: betas (0.9, 0.95), eps 1e-8,
// no weight decay, bias correction).  step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t); inv_scale un-scales grads.
// THE element update (adam_kernel, adam_multi_kernel's 16-byte walk); g is the un-scaled gradient.  adam_multi_kernel's scalar walk
// keeps the same lines written out: with a call there the compiler contracts b1 m + (1 - b1) g of the 16-BYTE walk into the other of
// its two possible fmas, and m changes in its last bit (LABNOTES, "Shared row-kernel rules: what could be written once").
__device__ __forceinline__ void adam_update(float g, float& m, float& v, float& p, float b1, float b2, float eps, float step_size,
                                            float bc2_sqrt) {
    const float mi = b1 * m + (1.f - b1) * g;
    const float vi = b2 * v + (1.f - b2) * g * g;
    m = mi;
    v = vi;
    p -= step_size * mi / (sqrtf(vi) / bc2_sqrt + eps);
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n, float b1, float b2, float eps, float step_size,
                            float bc2_sqrt, float inv_scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        adam_update(g[i] * inv_scale, m[i], v[i], p[i], b1, b2, eps, step_size, bc2_sqrt);
    }
}

// torch.optim.Adam over MANY tensors in one launch (torch's fused multi-tensor path needs 5 launches of ~45 us for the 160
// parameters of the depth-12 model, 1.3 TB/s; the update is 28 bytes per element of pure streaming).  items / chunks live
// in device memory: chunk c = elements [start, start + ADAM_CHUNK) of tensor chunks[c].item; one workgroup per chunk.
constexpr int ADAM_CHUNK = 4096;
__global__ __launch_bounds__(256) void adam_multi_kernel(const swv2_adam_item* __restrict__ items, const int2* __restrict__ chunks,
                                                         float b1, float b2, float eps, float step_size, float bc2_sqrt,
                                                         float inv_scale) {
    const int2 c = chunks[blockIdx.x];
    const swv2_adam_item it = items[c.x];
    const long lo = (long)c.y * ADAM_CHUNK, hi = min(it.n, lo + ADAM_CHUNK);
    float* __restrict__ p = it.p;
    const float* __restrict__ g = it.g;
    float* __restrict__ m = it.m;
    float* __restrict__ v = it.v;
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    if (vec) {
        for (long i = lo + 4 * threadIdx.x; i + 3 < hi; i += 4 * 256) {
            const f32x4 gi = *(const f32x4*)(g + i) * inv_scale;
            f32x4 mi = *(const f32x4*)(m + i), vi = *(const f32x4*)(v + i), pi = *(const f32x4*)(p + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float me = mi[e], ve = vi[e], pe = pi[e];          // (a reference cannot bind to a vector element)
                adam_update(gi[e], me, ve, pe, b1, b2, eps, step_size, bc2_sqrt);
                mi[e] = me; vi[e] = ve; pi[e] = pe;
            }
            *(f32x4*)(m + i) = mi; *(f32x4*)(v + i) = vi; *(f32x4*)(p + i) = pi;
        }
    }
    // scalar path: everything (unaligned tensors) or the tail of < 4 elements
    const long s0 = vec ? lo + ((hi - lo) & ~3L) : lo;
    for (long i = s0 + threadIdx.x; i < hi; i += 256) {
        const float gi = g[i] * inv_scale;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * mi / (sqrtf(vi) / bc2_sqrt + eps);
    }
}

template <int G, int CH>
void launch_ln_fwd(const swv2_ln_args* a, hipStream_t st) {
    const int rows_per_block = LN_BLOCK / G;
    const int grid = min(cdiv(a->M, rows_per_block), 256 * 16);
    hipLaunchKernelGGL((ln_residual_fwd_kernel<G, CH>), dim3(grid), dim3(LN_BLOCK), 0, st, (const uint16_t*)a->a, a->res,
                       a->gamma, a->beta, a->scale, a->rowidx, a->y, a->mean, a->rstd, a->M, a->C, a->res_mod,
                       a->rows_per_sample, a->eps);
}
template <int G, int CH>
void launch_ln_bwd(const swv2_ln_args* a, hipStream_t st) {
    const int rows_per_block = LN_BLOCK / G;
    const int grid = min(cdiv(a->M, rows_per_block), SWV2_LN_BWD_MAX_BLOCKS);
    hipLaunchKernelGGL((ln_residual_bwd_kernel<G, CH>), dim3(grid), dim3(LN_BLOCK), 0, st, (const uint16_t*)a->a, a->dy,
                       a->gamma, a->scale, a->rowidx, a->mean, a->rstd, (uint16_t*)a->da, a->ws, a->M, a->C,
                       a->rows_per_sample);
    hipLaunchKernelGGL(ln_partials_reduce_kernel, dim3(cdiv(2 * a->C, LNR_COLS)), dim3(LNR_COLS * LNR_SLICES), 0, st, a->ws,
                       a->dgamma, a->dbeta, grid, a->C, (const float*)nullptr, (float*)nullptr, (float*)nullptr, 0);
}

int ln_check(const swv2_ln_args* a, bool bwd) {
    SWV2_CHECK_ARG(a && a->a && a->gamma && a->mean && a->rstd, "ln_residual: null pointer");
    SWV2_CHECK_ARG(a->M > 0 && a->C > 0 && a->C % 8 == 0 && a->C <= 2048, "ln_residual: C=%d must be a multiple of 8, <= 2048", a->C);
    SWV2_CHECK_ARG(a->rows_per_sample > 0, "ln_residual: rows_per_sample must be positive");
    if (bwd) SWV2_CHECK_ARG(a->dy && a->da && a->dgamma && a->dbeta && a->ws, "ln_residual_bwd: null gradient / workspace pointer");
    else SWV2_CHECK_ARG(a->y && a->beta, "ln_residual_fwd: null output pointer");
    return SWV2_OK;
}

}  // namespace

// shared with mlp.hip (fused MLP backward): dgamma[j] += sum_b ws[b][0][j], dbeta[j] += sum_b ws[b][1][j]
void swv2_launch_ln_partials_reduce2(const float* ws1, float* dg1, float* db1, int n1, const float* ws2, float* dg2, float* db2,
                                     int n2, int C, hipStream_t st) {
    hipLaunchKernelGGL(ln_partials_reduce_kernel, dim3(cdiv(2 * C, LNR_COLS), 2), dim3(LNR_COLS * LNR_SLICES), 0, st, ws1, dg1, db1,
                       n1, C, ws2, dg2, db2, n2);
}

void swv2_launch_ln_partials_reduce(const float* ws, float* dgamma, float* dbeta, int nblocks, int C, hipStream_t st) {
    hipLaunchKernelGGL(ln_partials_reduce_kernel, dim3(cdiv(2 * C, LNR_COLS)), dim3(LNR_COLS * LNR_SLICES), 0, st, ws, dgamma,
                       dbeta, nblocks, C, (const float*)nullptr, (float*)nullptr, (float*)nullptr, 0);
}

#define LN_DISPATCH(FN)                                              \
    const int chunks = a->C / 8;                                     \
    if (chunks <= 16) FN<16, 1>(a, st);                              \
    else if (chunks <= 32) FN<32, 1>(a, st);                         \
    else if (chunks <= 64) FN<64, 1>(a, st);                         \
    else if (chunks <= 128) FN<64, 2>(a, st);                        \
    else FN<64, 4>(a, st);

extern "C" int swv2_ln_residual_fwd(const swv2_ln_args* a, void* stream) {
    int rc = ln_check(a, false);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    LN_DISPATCH(launch_ln_fwd)
    SWV2_CHECK_LAUNCH("swv2_ln_residual_fwd");
    return SWV2_OK;
}

extern "C" int swv2_ln_residual_bwd(const swv2_ln_args* a, void* stream) {
    int rc = ln_check(a, true);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    LN_DISPATCH(launch_ln_bwd)
    SWV2_CHECK_LAUNCH("swv2_ln_residual_bwd");
    return SWV2_OK;
}

// ------------------------------------------------------------------------------------------------
// second half of the q / k normalisation for the 96- / 128- / 256-wide head layouts (the GEMM epilogue leaves the squared norms in rnorm
// and the un-normalised values in qkvh, see heads_item_wide in gemm.hip): rn = 1 / max(|.|, 1e-12) (F.normalize's eps,
// swinv2_global.py:300-304), q, k rows rescaled in place, rnorm <- rn (0 on padded rows).  16 lanes per 128-wide row.
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void qk_normalize_kernel(uint16_t* __restrict__ qkvh, float* __restrict__ rnorm, long rows,
                                                           int h, int Lp, int L, int DP) {
    const long i = (long)blockIdx.x * 16 + (threadIdx.x >> 4);        // row index over [Bw][h][2][Lp]
    const int c = threadIdx.x & 15;                                   // 16-byte chunk of the row (DP / 8 of them: 12, 16 or 32)
    if (i >= rows) return;
    const int t = (int)(i % Lp);
    const long bh2 = i / Lp;
    const int part = (int)(bh2 & 1);
    const long bh = bh2 >> 1;
    const float ss = rnorm[i];
    const float rn = (t < L) ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 0.f;
    for (int cc = c; cc * 8 < DP; cc += 16) {                       // one chunk per lane at DP <= 128, two at 256
        uint16_t* row = qkvh + ((bh * 3 + part) * Lp + t) * DP + cc * 8;
        float v[8];
        unpack8(*(const uint4*)row, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= rn;
        *(uint4*)row = pack8(v);
    }
    if (c == 0) rnorm[i] = rn;
}
}  // namespace

extern "C" int swv2_qk_normalize(void* qkvh, float* rnorm, int Bw, int heads, int Lp, int L, int DP, void* stream) {
    SWV2_CHECK_ARG(qkvh && rnorm && Bw > 0 && heads > 0 && Lp > 0 && L > 0 && L <= Lp, "swv2_qk_normalize: bad argument");
    SWV2_CHECK_ARG(DP == 96 || DP == 128 || DP == 256, "swv2_qk_normalize: only the 96-, 128- and 256-wide head layouts need this pass (DP=%d)", DP);
    const long rows = (long)Bw * heads * 2 * Lp;
    hipLaunchKernelGGL(qk_normalize_kernel, dim3((unsigned)cdiv(rows, 16)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)qkvh,
                       rnorm, rows, heads, Lp, L, DP);
    SWV2_CHECK_LAUNCH("swv2_qk_normalize");
    return SWV2_OK;
}

extern "C" int swv2_prep_weight(const float* w, int rows, int cols, int transpose, const int32_t* row_map, int out_rows,
                                const int32_t* col_map, int out_cols, void* out_bf16, void* stream) {
    SWV2_CHECK_ARG(w && out_bf16 && rows > 0 && cols > 0 && out_rows > 0 && out_cols > 0, "prep_weight: bad argument");
    const long n = (long)out_rows * out_cols;
    hipLaunchKernelGGL(prep_weight_kernel, dim3(min(cdiv(n, 256), 4096)), dim3(256), 0, (hipStream_t)stream, w, rows, cols,
                       transpose, row_map, out_rows, col_map, out_cols, (uint16_t*)out_bf16);
    SWV2_CHECK_LAUNCH("swv2_prep_weight");
    return SWV2_OK;
}

extern "C" int swv2_prep_chunk(void) { return PREP_CHUNK; }

extern "C" int swv2_prep_item_chunks(int out_rows, int out_cols, int transpose) {
    if (out_rows <= 0 || out_cols <= 0) return 0;
    if (prep_tiled(out_rows, out_cols, transpose)) return ((out_rows + 63) / 64) * ((out_cols + 63) / 64);
    return (int)(((long)out_rows * out_cols + PREP_CHUNK - 1) / PREP_CHUNK);
}

extern "C" int swv2_prep_multi(const swv2_prep_item* items_dev, const int* chunks_dev, int n_chunks, void* stream) {
    SWV2_CHECK_ARG(items_dev && chunks_dev && n_chunks > 0, "prep_multi: bad argument");
    hipLaunchKernelGGL(prep_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, items_dev, (const int2*)chunks_dev);
    SWV2_CHECK_LAUNCH("swv2_prep_multi");
    return SWV2_OK;
}

extern "C" int swv2_batch_sum(const float* in, float* out, int B, long n, int accumulate, void* stream) {
    SWV2_CHECK_ARG(in && out && B > 0 && n > 0 && n % 4 == 0, "batch_sum: bad argument (n must be a multiple of 4)");
    hipLaunchKernelGGL(batch_sum_kernel, dim3(min(cdiv(n / 4, 256), 8192)), dim3(256), 0, (hipStream_t)stream, in, out, B, n,
                       accumulate);
    SWV2_CHECK_LAUNCH("swv2_batch_sum");
    return SWV2_OK;
}

extern "C" int swv2_merge_stats(const float* x, float* mean, float* rstd, int B, int H, int W, int C, float eps,
                                void* stream) {
    SWV2_CHECK_ARG(x && mean && rstd && B > 0 && H % 2 == 0 && W % 2 == 0 && C > 0, "merge_stats: bad argument");
    const long M = (long)B * (H / 2) * (W / 2);
    hipLaunchKernelGGL(merge_stats_kernel, dim3(min(cdiv(M, 4), 4096)), dim3(256), 0, (hipStream_t)stream, x, mean, rstd, B, H,
                       W, C, eps);
    SWV2_CHECK_LAUNCH("swv2_merge_stats");
    return SWV2_OK;
}

extern "C" int swv2_merge_ln_bwd(const float* x, const void* dn_bf16, const float* gamma, const float* mean,
                                 const float* rstd, float* dx, float* dgamma, float* dbeta, int B, int H, int W, int C,
                                 void* stream) {
    SWV2_CHECK_ARG(x && dn_bf16 && gamma && mean && rstd && dx && dgamma && dbeta, "merge_ln_bwd: null pointer");
    const long M = (long)B * (H / 2) * (W / 2);
    hipLaunchKernelGGL(merge_ln_bwd_kernel, dim3(min(cdiv(M, 4), 4096)), dim3(256), 0, (hipStream_t)stream, x,
                       (const uint16_t*)dn_bf16, gamma, mean, rstd, dx, dgamma, dbeta, B, H, W, C);
    SWV2_CHECK_LAUNCH("swv2_merge_ln_bwd");
    return SWV2_OK;
}

extern "C" int swv2_adam_chunk(void) { return ADAM_CHUNK; }

extern "C" int swv2_adam_multi(const swv2_adam_item* items_dev, const int* chunks_dev, int n_chunks, float lr, float beta1,
                               float beta2, float eps, int step, float grad_inv_scale, void* stream) {
    SWV2_CHECK_ARG(items_dev && chunks_dev && n_chunks > 0 && step > 0, "adam_multi: bad argument");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adam_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, items_dev, (const int2*)chunks_dev,
                       beta1, beta2, eps, lr / bc1, sqrtf(bc2), grad_inv_scale);
    SWV2_CHECK_LAUNCH("swv2_adam_multi");
    return SWV2_OK;
}

extern "C" int swv2_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                              float eps, int step, float grad_inv_scale, void* stream) {
    SWV2_CHECK_ARG(p && g && m && v && n > 0 && step > 0, "adam_step: bad argument");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adam_kernel, dim3(min(cdiv(n, 256), 8192)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, beta1,
                       beta2, eps, lr / bc1, sqrtf(bc2), grad_inv_scale);
    SWV2_CHECK_LAUNCH("swv2_adam_step");
    return SWV2_OK;
}
