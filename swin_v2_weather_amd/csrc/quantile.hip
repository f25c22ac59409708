// Order statistics of every (sample, channel) plane: the values at K given ranks of the sorted plane, for all planes and all ranks at
// once, without sorting.  Behind top_quantiles_error_torch (reference utils/weighted_acc_rmse.py:117-126): 100 quantile levels need at
// most 200 ranks, the same ones in every plane.  A multi-rank radix select over order-preserving 32-bit keys:
//
//     key = bits ^ 0xffffffff (negative), bits ^ 0x80000000 (non-negative), 0xffffffff (any NaN: NaNs sort last, as in torch.sort)
//
//   level  digit            count kernel                                   histogram in LDS
//     0    key[31:20]  12   quantile_count_kernel<0>   4 B/element         4096 x 4 B                      = 16 KB
//     1    key[19:15]   5   quantile_count_kernel<1>   4 B/element         256 slots x 32 x 4 B + prefixes = 33 KB
//     2    key[14:10]   5   quantile_count_kernel<2>        "                   "
//     3    key[ 9: 5]   5   quantile_count_kernel<3>        "                   "
//     4    key[ 4: 0]   5   quantile_count_kernel<4>        "                   "
//
// Launches of one swv2_plane_order_stats, all on the caller's stream, no host synchronisation in between:
//     memset(hist)   count<0> resolve   count<1> resolve   count<2> resolve   count<3> resolve   count<4> resolve(last)
//
// count<L>: workgroup (plane, slice) of the plan of plane_stream.h (workgroup index plane * slices + sl; an empty slice adds nothing)
// streams its slice with four 16-byte loads in flight per thread.  Level 0 counts the top digit of
// every element.  Level L > 0 looks the element's prefix key >> (25 - 5 L) up among the plane's active prefixes (at most K, sorted, held
// in LDS and padded to 256 with 0xffffffff: an 8-step lower bound) and counts its next digit into hist[slot][digit]; an element under
// no active prefix counts nowhere.  The lanes of a wave that hit the same counter as its first lane (all of them in a constant plane, most
// of them in a field of zeros, and -- the common case after level 1 -- all of them with no active prefix at all) add their number once
// instead of one by one.  The workgroup then adds its non-zero counters into the plane's histogram in the workspace with integer atomics.
//
// resolve (one workgroup per plane): inclusive prefix sum of the plane's histogram; every rank finds the counter that holds it (lower
// bound inside its slot) and keeps its residual inside that counter; the distinct (prefix << bits | digit) of the K ranks, ascending
// because the ranks are, become the active prefixes of the next level (never more than K).  It zeroes the plane's histogram for the
// next level.  Level 0 also stores the NaN count (counter 4095 holds the NaNs and nothing else); the last level's prefixes are whole
// keys and go to out[k][plane] as floats.
//
// Workspace per plane: 8192 counters (32 KB) + prefix[256] + slot[256] + residual[256] + 4 (nact) = 35 856 B.  The op zeroes the counters
// itself (one memset up front, resolve afterwards) and writes every state word before reading it: a dirty workspace gives the bits of a
// clean one.  Counters are integers: the result does not depend on the order in which workgroups or lanes arrive, two runs agree bit
// for bit.  One counter can hold a whole plane (H W < 2^30).
#include "plane_stream.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int Q_MAX_K = 256;
constexpr int Q_BITS0 = 12, Q_BITS = 5, Q_LEVELS = 5;
constexpr int Q_HIST = Q_MAX_K << Q_BITS;     // 8192 counters per plane: >= 1 << Q_BITS0
constexpr int Q_STATE = 3 * Q_MAX_K + 4;      // prefix[256], slot[256], residual[256], nact (+ 3 spare)
constexpr uint32_t Q_NONE = 0xffffffffu;

static_assert(Q_BITS0 + (Q_LEVELS - 1) * Q_BITS == 32, "the digits cover the key");
static_assert((1 << Q_BITS0) <= Q_HIST, "level 0 fits the plane's histogram");

__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}

__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

// one counter per active lane (id = Q_NONE: none); the lanes that name the counter of the wave's first active lane add their number once
__device__ __forceinline__ void wave_count(uint32_t* hist, uint32_t id) {
    const uint32_t first = __builtin_amdgcn_readfirstlane(id);
    const uint64_t same = __ballot(id == first);
    if (id == first) {
        if (first != Q_NONE && __lane_id() == __ffsll((unsigned long long)same) - 1) atomicAdd(hist + first, (uint32_t)__popcll(same));
    } else if (id != Q_NONE) {
        atomicAdd(hist + id, 1u);
    }
}

template <int LEVEL>
__device__ __forceinline__ uint32_t counter_of(uint32_t key, const uint32_t* pre) {
    if (LEVEL == 0) return key >> (32 - Q_BITS0);
    constexpr int sh = 32 - Q_BITS0 - LEVEL * Q_BITS;         // the digit's shift; the prefix is everything above the digit
    const uint32_t p = key >> (sh + Q_BITS);
    uint32_t pos = 0;
#pragma unroll
    for (int s = Q_MAX_K / 2; s > 0; s >>= 1) pos += pre[pos + s - 1] < p ? s : 0;
    return pre[pos] == p ? (pos << Q_BITS) | ((key >> sh) & ((1u << Q_BITS) - 1)) : Q_NONE;
}

template <int LEVEL>
__device__ __forceinline__ void count_vec(const f32x4 v, uint32_t* hist, const uint32_t* pre) {
#pragma unroll
    for (int e = 0; e < 4; ++e) wave_count(hist, counter_of<LEVEL>(float_key(v[e]), pre));
}

template <int LEVEL>
__global__ __launch_bounds__(256) void quantile_count_kernel(const float* __restrict__ x, long bstride, int C, int H, int W, int slices,
                                                             uint32_t* __restrict__ ws) {
    constexpr int NH = LEVEL == 0 ? (1 << Q_BITS0) : Q_HIST;
    __shared__ uint32_t hist[NH];
    __shared__ uint32_t pre[LEVEL == 0 ? 1 : Q_MAX_K];
    const int pl = blockIdx.x / slices, sl = blockIdx.x - pl * slices, b = pl / C, c = pl - b * C;
    uint32_t* ghist = ws + (size_t)pl * (Q_HIST + Q_STATE);
    const uint32_t* state = ghist + Q_HIST;
    int n = NH;
    if (LEVEL > 0) {
        int nact = (int)state[3 * Q_MAX_K];                   // 1 .. K, written by the resolve before
        nact = nact < 0 ? 0 : (nact > Q_MAX_K ? Q_MAX_K : nact);
        n = nact << Q_BITS;
        pre[threadIdx.x] = (int)threadIdx.x < nact ? state[threadIdx.x] : Q_NONE;
    }
    for (int i = threadIdx.x; i < n; i += 256) hist[i] = 0;
    __syncthreads();
    const uint32_t plane = (uint32_t)H * W;                   // < 2^30, a multiple of 4 (checked by the host)
    uint32_t lo, hi;
    plane_slice_range(plane, sl, slices, lo, hi);
    const float* p = x + b * bstride + (long)c * plane;
    uint32_t i = lo + threadIdx.x * 4;
    for (; i + 3 * 1024 < hi; i += 4 * 1024) {
        f32x4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = *(const f32x4*)(p + i + u * 1024);
#pragma unroll
        for (int u = 0; u < 4; ++u) count_vec<LEVEL>(a[u], hist, pre);
    }
    for (; i < hi; i += 1024) count_vec<LEVEL>(*(const f32x4*)(p + i), hist, pre);
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 256) {
        const uint32_t v = hist[j];
        if (v) atomicAdd(ghist + j, v);
    }
}

// inclusive sum over the 256 threads of the workgroup; sm: 4 words of LDS, free again after the call
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sm) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    if (lane == 63) sm[wv] = v;
    __syncthreads();
    for (int u = 0; u < wv; ++u) v += sm[u];
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(256) void quantile_resolve_kernel(uint32_t* __restrict__ ws, const int* __restrict__ ranks, int K, int level,
                                                               int planes, float* __restrict__ out, int* __restrict__ nan_count) {
    __shared__ uint32_t cum[Q_HIST];
    __shared__ uint32_t np[Q_MAX_K];
    __shared__ uint32_t sm[4];
    const int pl = blockIdx.x, t = threadIdx.x;
    uint32_t* ghist = ws + (size_t)pl * (Q_HIST + Q_STATE);
    uint32_t* prefix = ghist + Q_HIST;
    uint32_t* slot = prefix + Q_MAX_K;
    uint32_t* resid = slot + Q_MAX_K;
    const int nd = level == 0 ? (1 << Q_BITS0) : (1 << Q_BITS);
    int nact = level == 0 ? 1 : (int)prefix[3 * Q_MAX_K];
    nact = nact < 1 ? 1 : (nact > Q_MAX_K ? Q_MAX_K : nact);
    const int n = nact * nd;                                   // <= Q_HIST
    for (int i = t; i < n; i += 256) cum[i] = ghist[i];
    __syncthreads();
    for (int i = t; i < Q_HIST / 4; i += 256) *(u32x4*)(ghist + 4 * i) = u32x4{0u, 0u, 0u, 0u};          // for the next level
    // thread t sums the counters [t per, (t + 1) per), the workgroup scans the 256 sums, the thread writes its running sums back
    const int per = (n + 255) / 256, i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
    uint32_t s = 0;
    for (int i = i0; i < i1; ++i) s += cum[i];
    uint32_t run = block_scan(s, sm) - s;
    for (int i = i0; i < i1; ++i) { run += cum[i]; cum[i] = run; }
    __syncthreads();
    if (level == 0 && t == 0) nan_count[pl] = (int)(cum[4095] - cum[4094]);
    uint32_t newp = 0, newr = 0;
    if (t < K) {
        int sk = 0;
        uint32_t r = (uint32_t)ranks[t], pk = 0;
        if (level > 0) {
            sk = (int)slot[t];
            sk = sk < nact ? sk : nact - 1;
            r = resid[t];
            pk = prefix[sk];
        }
        const int base = sk * nd;
        const uint32_t target = (base ? cum[base - 1] : 0u) + r;
        int a = base, e = base + nd - 1;                       // the smallest i in [base, base + nd - 1] with cum[i] > target (else the last)
        while (a < e) {
            const int m = (a + e) >> 1;
            if (cum[m] > target) e = m; else a = m + 1;
        }
        newr = target - (a ? cum[a - 1] : 0u);
        newp = level == 0 ? (uint32_t)a : (pk << Q_BITS) | (uint32_t)(a - base);
        np[t] = newp;
    }
    __syncthreads();                                           // every read of the old state is done
    if (level == Q_LEVELS - 1) {
        if (t < K) out[(size_t)t * planes + pl] = key_float(newp);
        return;
    }
    const uint32_t flag = t < K && (t == 0 || np[t - 1] != newp) ? 1u : 0u;
    const uint32_t pos = block_scan(flag, sm);                 // ranks ascend, so do their prefixes: equal ones are neighbours
    if (t < K) {
        if (flag) prefix[pos - 1] = newp;
        slot[t] = pos - 1;
        resid[t] = newr;
    }
    if (t == 255) prefix[3 * Q_MAX_K] = pos;
}

template <int LEVEL>
void launch_count(const float* x, long bstride, int planes, int C, int H, int W, int slices, uint32_t* ws, hipStream_t st) {
    hipLaunchKernelGGL(quantile_count_kernel<LEVEL>, dim3((unsigned)((long)planes * slices)), dim3(256), 0, st, x, bstride, C, H, W, slices, ws);
}

}  // namespace

extern "C" size_t swv2_quantile_ws_bytes(int planes, int H, int W, int K) {
    if (planes <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    return (size_t)planes * (Q_HIST + Q_STATE) * sizeof(uint32_t);
}

extern "C" int swv2_plane_order_stats(const float* x, long bstride, int B, int C, int H, int W, const int* ranks, int K, float* out,
                                      int* nan_count, void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(x && ranks && out && nan_count && ws, "plane_order_stats: null pointer");
    SWV2_CHECK_ARG(B > 0 && C > 0 && plane_shape_ok((long)B * C, H, W), "plane_order_stats: bad shape (B, C, H, W > 0, B * C < 2^20, H * W < 2^30)");
    SWV2_CHECK_ARG((long)H * W % 4 == 0, "plane_order_stats: H * W % 4 != 0");
    SWV2_CHECK_ARG(K >= 1 && K <= Q_MAX_K, "plane_order_stats: K outside 1 .. 256");
    SWV2_CHECK_ARG((((uintptr_t)ranks | (uintptr_t)out | (uintptr_t)nan_count) & 3) == 0,
                   "plane_order_stats: pointer not 4-byte aligned (ranks, out, nan_count)");
    const int planes = B * C;
    if (!plane_operands_ok("plane_order_stats", {x, ws}, {bstride}, B, (long)C * H * W, ws_bytes, swv2_quantile_ws_bytes(planes, H, W, K),
                           "swv2_quantile_ws_bytes"))
        return SWV2_ERR_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const int slices = plane_slices(planes);
    uint32_t* w = (uint32_t*)ws;
    if (hipMemsetAsync(w, 0, (size_t)planes * (Q_HIST + Q_STATE) * sizeof(uint32_t), st) != hipSuccess) {
        swv2_set_error("plane_order_stats: hipMemsetAsync failed");
        return SWV2_ERR_LAUNCH;
    }
    for (int level = 0; level < Q_LEVELS; ++level) {
        switch (level) {
            case 0: launch_count<0>(x, bstride, planes, C, H, W, slices, w, st); break;
            case 1: launch_count<1>(x, bstride, planes, C, H, W, slices, w, st); break;
            case 2: launch_count<2>(x, bstride, planes, C, H, W, slices, w, st); break;
            case 3: launch_count<3>(x, bstride, planes, C, H, W, slices, w, st); break;
            default: launch_count<4>(x, bstride, planes, C, H, W, slices, w, st); break;
        }
        SWV2_CHECK_LAUNCH("swv2_plane_order_stats (count)");
        hipLaunchKernelGGL(quantile_resolve_kernel, dim3(planes), dim3(256), 0, st, w, ranks, K, level, planes, out, nan_count);
        SWV2_CHECK_LAUNCH("swv2_plane_order_stats (resolve)");
    }
    return SWV2_OK;
}
