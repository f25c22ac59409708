// LAMB (apex FusedLAMB semantics, reference train.py:177-178) over MANY fp32 tensors: the multi-tensor shape of adam_multi_kernel
// (rowops.hip) -- item and chunk tables in device memory, one 256-thread workgroup per LAMB_CHUNK elements, 16-byte accesses
// where p, g, m and v are all 16-byte aligned, single-element accesses for unaligned tensors and tails (same walk, same sums).
//
//   launch 0 (once per step, all groups)  lamb_gsq_kernel     4 B/element   per-chunk partial sums of (g * grad_inv_scale)^2
//   per group:
//   launch 1  lamb_clip_kernel    one workgroup: ||g||^2 over ALL chunk partials (+ the caller's share), clip divisor c, bc1, bc2
//   launch 2  lamb_stage1_kernel  24 B/element  reads p g m v, writes m v, per-chunk partial sums of p^2 and u^2
//   launch 3  lamb_norms_kernel   one workgroup per tensor: ||p||^2, ||u||^2, trust ratio r
//   launch 4  lamb_stage2_kernel  16 B/element  reads p m v, writes p <- p - lr r u
// g is only ever read (it may be a DDP bucket view or the accumulation target of a rollout; apex overwrites it with u): stage 2
// recomputes u from the stored m, v and the old p through lamb_update(), the one statement of u that stage 1 calls too.
//
// Sums: no float atomics; the order is fixed by the tables alone, so two runs from the same state agree bit for bit.  On its way
// into a norm the square of an element passes through at most D = SWV2_LAMB_SUM_DEPTH = 64 fp32 additions:
//     17  the thread's own running sum (16 elements of a chunk + at most one element of a partial chunk's tail)
//      6  wave64 butterfly
//      2  the four waves through LDS, (w0 + w1) + (w2 + w3)                                   = 25 for a chunk partial
//      h  tree_sum: pairwise halving passes over the chunk partials until LAMB_TREE_LEAF = 2048 are left; h <= 20 for n_chunks < 2^31
//      8  the thread's own sum of its 2048 / 256 leaves
//    6+2  butterfly and LDS again
//      1  the caller's share of ||g||^2 (swv2_lamb_multi's extra_gnorm2)                     = 62 at most
#include "common.h"

namespace {

constexpr int LAMB_CHUNK = 4096;
constexpr int LAMB_TREE_LEAF = 2048;

struct LambArgs {        // what the caller passed, every scalar as fp32
    float lr, b1, b2, eps, wd, bc1, bc2, inv_scale, max_norm;
    int flags;
};

// per-launch constants derived from LambArgs in fp32 (1 - beta is exact for beta in [0.5, 1])
struct LambK {
    float b1, b2, b3, omb2, eps, wd, rbc1, rbc2, gs;
    double gs_d;
    bool adamw;
    // head: the workspace's, written by lamb_clip_kernel.  gs = inv_scale / c in fp32; gs_d the same from |g|^2 in fp64 (L2 mode)
    __device__ __forceinline__ LambK(const LambArgs& a, const float* head)
        : b1(a.b1), b2(a.b2), b3((a.flags & SWV2_LAMB_GRAD_AVERAGING) ? 1.f - a.b1 : 1.f), omb2(1.f - a.b2), eps(a.eps), wd(a.wd),
          rbc1(1.f / a.bc1), rbc2(1.f / a.bc2), gs(a.inv_scale / head[SWV2_LAMB_WS_CLIP]),
          gs_d((a.flags & SWV2_LAMB_ADAMW)           ? 0.0          // (not read in adam_w_mode)
               : head[SWV2_LAMB_WS_CLIP] == 1.f ? (double)a.inv_scale
                                                : (double)a.inv_scale * (double)a.max_norm / sqrt((double)head[SWV2_LAMB_WS_GNORM2])),
          adamw((a.flags & SWV2_LAMB_ADAMW) != 0) {}
};

// u of one element from the NEW moments and the OLD parameter: the only statement of it, called by both stages
__device__ __forceinline__ float lamb_update(float m, float v, float p, const LambK& k) {
    const float a = (m * k.rbc1) / (sqrtf(v * k.rbc2) + k.eps);
    return k.adamw ? fmaf(k.wd, p, a) : a;
}

// new moments of one element.  L2 mode forms g^ = g s + wd p in fp64 and rounds once: the two terms cancel freely, and the error of
// an fp32 g s would then be large against g^ itself (adam_w_mode has no sum there, fp32 is enough)
__device__ __forceinline__ void lamb_moments(float g, float p, float& m, float& v, const LambK& k) {
    const float gh = k.adamw ? g * k.gs : (float)fma((double)k.wd, (double)p, (double)g * k.gs_d);
    m = k.b1 * m + k.b3 * gh;
    v = k.b2 * v + (k.omb2 * gh) * gh;
}

// W elements at p: one 16-byte access where `vec` (W = 4 and all four tensors aligned), else single elements
template <int W>
__device__ __forceinline__ void ldw(const float* p, float (&x)[W], bool vec) {
    if constexpr (W == 4) {
        if (vec) {
            const f32x4 t = *(const f32x4*)p;
            x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) x[e] = p[e];
}
template <int W>
__device__ __forceinline__ void stw(float* p, const float (&x)[W], bool vec) {
    if constexpr (W == 4) {
        if (vec) {
            const f32x4 t = {x[0], x[1], x[2], x[3]};
            *(f32x4*)p = t;
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) p[e] = x[e];
}

// f(i, width) over the elements [lo, hi) of one chunk: groups of four, then the tail of < 4 single elements.  The same thread takes the
// same elements in the same order whether the tensors are aligned or not (ldw / stw differ, the walk does not), so the sums do not depend
// on where an allocator put a buffer.  A thread sees at most 16 elements in groups and, then, at most one of the tail (a tail exists only
// below a full chunk)
template <class F>
__device__ __forceinline__ void chunk_walk(long lo, long hi, F f) {
    for (long i = lo + 4 * threadIdx.x; i + 3 < hi; i += 4 * 256) f(i, std::integral_constant<int, 4>{});
    for (long i = lo + ((hi - lo) & ~3L) + threadIdx.x; i < hi; i += 256) f(i, std::integral_constant<int, 1>{});
}

// sum over the 256 threads of a workgroup, the same value in every thread: butterfly, then (w0 + w1) + (w2 + w3)
__device__ __forceinline__ float block_sum(float s, float* lds) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    const float r = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return r;
}

// part[0 .. n) summed by one workgroup in a fixed order of logarithmic depth: halving passes part -> scr -> scr (element i takes
// i + half) until LAMB_TREE_LEAF values are left, then 8 per thread.  part is left as it was; scr holds (n + 1) / 2 floats.
__device__ float tree_sum(const float* part, float* scr, int n, float* lds) {
    const float* src = part;
    while (n > LAMB_TREE_LEAF) {
        const int half = (n + 1) >> 1;
        for (int i = threadIdx.x; i < half; i += 256) scr[i] = i + half < n ? src[i] + src[i + half] : src[i];
        __syncthreads();            // (a workgroup-scope fence: the next pass reads what other waves stored)
        src = scr;
        n = half;
    }
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += src[i];
    return block_sum(s, lds);
}

struct LambChunk {
    swv2_lamb_item it;
    long lo, hi;
    long slot;          // of this chunk's partial sums
    int item;
    bool vec;
    __device__ __forceinline__ LambChunk(const swv2_lamb_item* items, const int2* chunks, int chunk) {
        const int2 c = chunks[chunk];
        item = c.x;
        it = items[c.x];
        lo = (long)c.y * LAMB_CHUNK;
        hi = min(it.n, lo + LAMB_CHUNK);
        slot = it.chunk0 + c.y;
        vec = ((((uintptr_t)it.p | (uintptr_t)it.g | (uintptr_t)it.m | (uintptr_t)it.v) & 15) == 0);
    }
};

__global__ __launch_bounds__(256) void lamb_gsq_kernel(const swv2_lamb_item* __restrict__ items, const int2* __restrict__ chunks,
                                                       int n_chunks, float inv_scale, float* __restrict__ g_part) {
    __shared__ float lds[4];
    const LambChunk c(items, chunks, blockIdx.x);
    const float* __restrict__ g = c.it.g;
    float s = 0.f;
    chunk_walk(c.lo, c.hi, [&](long i, auto W) {
        float x[decltype(W)::value];
        ldw(g + i, x, c.vec);
#pragma unroll
        for (int e = 0; e < decltype(W)::value; ++e) {
            const float t = x[e] * inv_scale;
            s += t * t;
        }
    });
    s = block_sum(s, lds);
    if (threadIdx.x == 0 && c.slot < n_chunks) g_part[c.slot] = s;
}

__global__ __launch_bounds__(256) void lamb_clip_kernel(const float* g_part, float* g_scr, int n_chunks, const float* __restrict__ extra,
                                                        float max_norm, float bc1, float bc2, float* __restrict__ head) {
    __shared__ float lds[4];
    float g2 = tree_sum(g_part, g_scr, n_chunks, lds);
    if (threadIdx.x == 0) {
        if (extra) g2 += *extra;
        const float G = sqrtf(g2);
        head[SWV2_LAMB_WS_GNORM2] = g2;
        head[SWV2_LAMB_WS_CLIP] = G > max_norm ? G / max_norm : 1.f;
        head[SWV2_LAMB_WS_BC1] = bc1;
        head[SWV2_LAMB_WS_BC2] = bc2;
    }
}

__global__ __launch_bounds__(256) void lamb_stage1_kernel(const swv2_lamb_item* __restrict__ items, const int2* __restrict__ chunks,
                                                          int chunk_lo, int n_chunks, LambArgs a, const float* __restrict__ head,
                                                          float* __restrict__ p_part, float* __restrict__ u_part) {
    __shared__ float lds[4];
    const LambChunk c(items, chunks, chunk_lo + blockIdx.x);
    const LambK k(a, head);
    const float* __restrict__ p = c.it.p;
    const float* __restrict__ g = c.it.g;
    float* __restrict__ m = c.it.m;
    float* __restrict__ v = c.it.v;
    float sp = 0.f, su = 0.f;
    chunk_walk(c.lo, c.hi, [&](long i, auto W) {
        constexpr int w = decltype(W)::value;
        float pi[w], gi[w], mi[w], vi[w];
        ldw(p + i, pi, c.vec); ldw(g + i, gi, c.vec); ldw(m + i, mi, c.vec); ldw(v + i, vi, c.vec);
#pragma unroll
        for (int e = 0; e < w; ++e) {
            lamb_moments(gi[e], pi[e], mi[e], vi[e], k);
            const float u = lamb_update(mi[e], vi[e], pi[e], k);
            sp += pi[e] * pi[e];
            su += u * u;
        }
        stw(m + i, mi, c.vec); stw(v + i, vi, c.vec);
    });
    sp = block_sum(sp, lds);
    su = block_sum(su, lds);
    if (threadIdx.x == 0 && c.slot < n_chunks) {
        p_part[c.slot] = sp;
        u_part[c.slot] = su;
    }
}

// one workgroup per tensor of the group: its chunk partials -> ||p||^2, ||u||^2 and the trust ratio
__global__ __launch_bounds__(256) void lamb_norms_kernel(const swv2_lamb_item* __restrict__ items, int item_lo, int n_chunks,
                                                         const float* p_part, float* p_scr, const float* u_part, float* u_scr,
                                                         int use_ratio, float* __restrict__ head) {
    __shared__ float lds[4];
    const int item = item_lo + blockIdx.x;
    const swv2_lamb_item it = items[item];
    const long nc = (it.n + LAMB_CHUNK - 1) / LAMB_CHUNK;
    if (it.chunk0 < 0 || it.chunk0 + nc > n_chunks) return;        // (a table that does not fit the workspace: touch nothing)
    const float p2 = tree_sum(p_part + it.chunk0, p_scr + it.chunk0, (int)nc, lds);
    const float u2 = tree_sum(u_part + it.chunk0, u_scr + it.chunk0, (int)nc, lds);
    if (threadIdx.x == 0) {
        float* o = head + SWV2_LAMB_WS_ITEM(item);
        o[0] = p2;
        o[1] = u2;
        o[2] = (use_ratio && p2 != 0.f && u2 != 0.f) ? sqrtf(p2) / sqrtf(u2) : 1.f;
    }
}

__global__ __launch_bounds__(256) void lamb_stage2_kernel(const swv2_lamb_item* __restrict__ items, const int2* __restrict__ chunks,
                                                          int chunk_lo, LambArgs a, const float* __restrict__ head) {
    const LambChunk c(items, chunks, chunk_lo + blockIdx.x);
    const LambK k(a, head);
    const float lrr = a.lr * head[SWV2_LAMB_WS_ITEM(c.item) + 2];
    float* __restrict__ p = c.it.p;
    const float* __restrict__ m = c.it.m;
    const float* __restrict__ v = c.it.v;
    chunk_walk(c.lo, c.hi, [&](long i, auto W) {
        constexpr int w = decltype(W)::value;
        float pi[w], mi[w], vi[w];
        ldw(p + i, pi, c.vec); ldw(m + i, mi, c.vec); ldw(v + i, vi, c.vec);
#pragma unroll
        for (int e = 0; e < w; ++e) pi[e] -= lrr * lamb_update(mi[e], vi[e], pi[e], k);
        stw(p + i, pi, c.vec);
    });
}

// the workspace, in floats: head | 4 per item | g, p, u chunk partials and one halving scratch each
struct LambWs {
    float *head, *g_part, *g_scr, *p_part, *p_scr, *u_part, *u_scr;
    LambWs(void* ws, int n_items, int n_chunks) {
        head = (float*)ws;
        g_part = head + SWV2_LAMB_WS_ITEM(n_items);
        g_scr = g_part + n_chunks; p_part = g_scr + n_chunks; p_scr = p_part + n_chunks; u_part = p_scr + n_chunks; u_scr = u_part + n_chunks;
    }
};

int lamb_check_tables(const char* who, const void* items, const void* chunks, int n_items, int n_chunks, const void* ws, size_t ws_bytes) {
    SWV2_CHECK_ARG(items && chunks, "%s: null item / chunk table", who);
    SWV2_CHECK_ARG(n_items > 0 && n_chunks > 0, "%s: n_items=%d, n_chunks=%d must be positive", who, n_items, n_chunks);
    SWV2_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "%s: null or unaligned workspace", who);
    SWV2_CHECK_ARG(ws_bytes >= swv2_lamb_ws_bytes(n_items, n_chunks), "%s: workspace of %zu bytes, swv2_lamb_ws_bytes(%d, %d) = %zu", who,
                   ws_bytes, n_items, n_chunks, swv2_lamb_ws_bytes(n_items, n_chunks));
    return SWV2_OK;
}

}  // namespace

extern "C" int swv2_lamb_chunk(void) { return LAMB_CHUNK; }

extern "C" size_t swv2_lamb_ws_bytes(int n_items, int n_chunks) {
    if (n_items <= 0 || n_chunks <= 0) return 0;
    return sizeof(float) * ((size_t)SWV2_LAMB_WS_ITEM(n_items) + 6 * (size_t)n_chunks);
}

extern "C" int swv2_lamb_grad_norm(const swv2_lamb_item* items_dev, const int* chunks_dev, int n_items, int n_chunks, float grad_inv_scale,
                                   void* ws, size_t ws_bytes, void* stream) {
    if (int rc = lamb_check_tables("lamb_grad_norm", items_dev, chunks_dev, n_items, n_chunks, ws, ws_bytes)) return rc;
    const LambWs w(ws, n_items, n_chunks);
    hipLaunchKernelGGL(lamb_gsq_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, items_dev, (const int2*)chunks_dev, n_chunks,
                       grad_inv_scale, w.g_part);
    SWV2_CHECK_LAUNCH("swv2_lamb_grad_norm");
    return SWV2_OK;
}

extern "C" int swv2_lamb_multi(const swv2_lamb_item* items_dev, const int* chunks_dev, int n_items, int n_chunks, int item_lo, int item_hi,
                               int chunk_lo, int chunk_hi, float lr, float beta1, float beta2, float eps, float weight_decay,
                               float grad_inv_scale, float max_grad_norm, int step, int flags, const float* extra_gnorm2, void* ws,
                               size_t ws_bytes, void* stream) {
    if (int rc = lamb_check_tables("lamb_multi", items_dev, chunks_dev, n_items, n_chunks, ws, ws_bytes)) return rc;
    SWV2_CHECK_ARG(0 <= item_lo && item_lo < item_hi && item_hi <= n_items, "lamb_multi: items [%d, %d) of %d", item_lo, item_hi, n_items);
    SWV2_CHECK_ARG(0 <= chunk_lo && chunk_lo < chunk_hi && chunk_hi <= n_chunks, "lamb_multi: chunks [%d, %d) of %d", chunk_lo, chunk_hi,
                   n_chunks);
    SWV2_CHECK_ARG(step >= 1, "lamb_multi: step=%d must be at least 1", step);
    SWV2_CHECK_ARG((flags & ~(SWV2_LAMB_ADAMW | SWV2_LAMB_BIAS_CORRECTION | SWV2_LAMB_GRAD_AVERAGING | SWV2_LAMB_NVLAMB)) == 0,
                   "lamb_multi: unknown flag bits 0x%x", flags);
    const bool bc = (flags & SWV2_LAMB_BIAS_CORRECTION) != 0;
    LambArgs a;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay; a.inv_scale = grad_inv_scale; a.max_norm = max_grad_norm;
    a.bc1 = bc ? (float)(1.0 - pow((double)beta1, (double)step)) : 1.f;
    a.bc2 = bc ? (float)(1.0 - pow((double)beta2, (double)step)) : 1.f;
    a.flags = flags;
    const LambWs w(ws, n_items, n_chunks);
    const hipStream_t st = (hipStream_t)stream;
    const int2* chunks = (const int2*)chunks_dev;
    const int use_ratio = (flags & SWV2_LAMB_NVLAMB) != 0 || weight_decay != 0.f;
    hipLaunchKernelGGL(lamb_clip_kernel, dim3(1), dim3(256), 0, st, w.g_part, w.g_scr, n_chunks, extra_gnorm2, a.max_norm, a.bc1, a.bc2, w.head);
    hipLaunchKernelGGL(lamb_stage1_kernel, dim3(chunk_hi - chunk_lo), dim3(256), 0, st, items_dev, chunks, chunk_lo, n_chunks, a,
                       (const float*)w.head, w.p_part, w.u_part);
    hipLaunchKernelGGL(lamb_norms_kernel, dim3(item_hi - item_lo), dim3(256), 0, st, items_dev, item_lo, n_chunks, w.p_part, w.p_scr,
                       w.u_part, w.u_scr, use_ratio, w.head);
    hipLaunchKernelGGL(lamb_stage2_kernel, dim3(chunk_hi - chunk_lo), dim3(256), 0, st, items_dev, chunks, chunk_lo, a, (const float*)w.head);
    SWV2_CHECK_LAUNCH("swv2_lamb_multi");
    return SWV2_OK;
}
