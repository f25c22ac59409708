// Shared pieces of the GEMM engine: tile constants, LDS swizzle, GELU, the head-major window layout, operand loaders, host checks.
// Included by every engine source: gemm.hip (the 128-row NT tile kernel, kernel selection, swv2_linear), gemm_wide.hip (256 x 256 NT
// kernels), gemm_rw.hip (the resident-weight row GEMMs of a block), gemm_tn.hip / gemm_tn_wide.hip / gemm_tn_slab.hip (weight gradients), and by the fused
// kernels (mlp.hip, proj_ln.hip).  The epilogues of the NT products are in gemm_epilogue.h.
#pragma once
#include <cstdlib>
#include "common.h"

// Kernels that gemm.hip's launch_nt2 selects (linear_kernel_for) and another source holds; the selector has checked the shapes.
// gemm_rw.hip: the resident-weight qkv product (parts = 1: LinearKernel::RESIDENT_QKV128, N = 384, K = 128; parts = 3: RESIDENT_QKV192X3, one
// launch per q / k / v part, N = 3 x 256, K = 192) and the streaming body of the d(qkv) -> dx product at C = 128 (RESIDENT_DX128)
int swv2_rw_qkv_launch(int parts, const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, hipStream_t st);
int swv2_rw_dx128_launch(const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, hipStream_t st);
// gemm_wide.hip: the 256 x 256 kernels (LinearKernel::WIDE_DMA: dma = true, WIDE) for the internal kinds (ak, ek) of a wide_pair
int swv2_nt_wide_launch(int ak, int ek, bool dma, const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, int N, int K, hipStream_t st);

// gemm_tn_wide.hip: one weight gradient on 256 x 256 tiles (WgradKernel::WIDE).  gemm_tn.hip's selector needs only the bytes of workspace
// the wide plan wants for (M, N, K), 0 = shape not covered; the launch is for an item and a workspace the selector accepted
size_t swv2_tn_wide_ws_bytes(int M, int N, int K);
int swv2_tn_wide_launch(const swv2_wgrad_item& it, void* ws, hipStream_t st);

// gemm_tn_slab.hip: the block's four weight gradients with every operand byte fetched once (LDS-DMA slabs).  swv2_tn_slab_covers: the
// kernel runs these items with a workspace of ws_bytes on `cus` CUs (0: the current device's, 256 assumed in a process without one),
// and, where it does, *plan (optional) receives the slices, stage rows, workgroups and bytes; a covered shape with too small a workspace
// is reported on stderr once per process.  swv2_block_wgrad asks it, then launches (0 or a negative error)
size_t swv2_tn_slab_ws_bytes(int C, int hidden, int heads_dp);
bool swv2_tn_slab_covers(const swv2_wgrad_item* it, size_t ws_bytes, int cus, swv2_block_wgrad_plan_t* plan);
int swv2_tn_slab_launch(const swv2_wgrad_item* it, void* ws, size_t ws_bytes, const swv2_ln_partials* ln, hipStream_t st);

// The two run-time switches of the GEMM engine, each parsed here and nowhere else; read per call (the tests toggle them in-process).
// SWV2_GEMM_WIDE (default 1): 0 = the 128-row tile kernels where swv2_linear / swv2_linear_wgrad_ws would run a 256 x 256 kernel.
// SWV2_WIDE_PERSIST (default 1): 0 = one workgroup per tile in the wide LDS-DMA kernel instead of persistent workgroups.
inline int swv2_env_switch(const char* name) { const char* v = getenv(name); return v ? atoi(v) : 1; }
inline int swv2_gemm_wide() { return swv2_env_switch("SWV2_GEMM_WIDE"); }
inline int swv2_wide_persist() { return swv2_env_switch("SWV2_WIDE_PERSIST"); }

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int KCH = BK / 8;                 // 16-byte chunks per tile row
constexpr int NTHREADS = 256;
// the 256 x 256 tile kernels (gemm_wide.hip; the wide weight-gradient kernel of gemm_tn_wide.hip): 8 waves, four LDS-DMA stage slots of
// (256 + 256) rows x 32 k (32 KB each) + a 2 KB pad behind the last (the epilogue's staging = slot 3 + pad)
constexpr int WBM = 256, WBN = 256, WTH = 512;
constexpr int WSTG = (WBM + WBN) * 32;                 // elements per stage slot
constexpr int WSM_BYTES = 4 * WSTG * 2 + 2048;

// XOR swizzle of bf16 tiles whose rows are whole 128-byte lines: the 16-byte chunk kc of row r sits at physical chunk swz_chunk(r, kc)
// (conflict-free ds_read_b128 of MFMA fragments)
__device__ __forceinline__ int swz_chunk(int r, int kc) { return kc ^ ((r >> 1) & 7); }
// swizzled element offset of chunk kc of row r in a [rows][64] bf16 tile (128-byte rows)
__device__ __forceinline__ int swz(int r, int kc) { return r * BK + (swz_chunk(r, kc) << 3); }

// erf-GELU (timm Mlp act = nn.GELU) with the Abramowitz-Stegun 7.1.26 rational erf (|err| < 1.5e-7, far below the
// bf16 storage precision): one v_rcp + one v_exp + a few FMAs instead of the ~40-instruction erff().
__device__ __forceinline__ void erf_parts(float x, float& erf_v, float& gauss) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.f));
    gauss = __expf(-z * z);                                    // exp(-x^2 / 2)
    const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
    const float e = fmaf(-poly, gauss, 1.f);
    erf_v = copysignf(e, x);
}
// exact unsigned division by a runtime-constant divisor d with magic = ceil(2^32 / d) (host: fdiv_magic): the estimate
// umulhi(n, magic) is q or q + 1 for every n < 2^32, one compare fixes it.  Replaces ~25-instruction integer divides
// in the loaders' index math (row -> (window, token), column -> (part, head)).
__device__ __forceinline__ int fdiv(int n, int d, uint32_t magic) {
    int q = (int)__umulhi((uint32_t)n, magic);
    return q - (q * d > n);
}
static inline uint32_t fdiv_magic(int d) { return d > 1 ? (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d) : 0u; }

__device__ __forceinline__ float gelu_f(float x) {
    float e, gs;
    erf_parts(x, e, gs);
    return 0.5f * x * (1.f + e);
}
__device__ __forceinline__ float gelu_grad_f(float x) {
    float e, gs;
    erf_parts(x, e, gs);
    return fmaf(x * 0.3989422804014327f, gs, 0.5f * (1.f + e));
}

// ------------------------------------------------------------------------------------------------
// Table-driven GELU for bf16 inputs.  The argument of every GELU / GELU' on this path is a STORED bf16 pre-activation, so
// the function has at most 65536 distinct arguments; for |x| in [2^-14, 2^4) (18 binades x 128 mantissas x 2 signs =
// 4608 entries) the value is looked up in an LDS table that each workgroup fills once with the formulas above -- the
// results are bit-identical to evaluating them per element (~14 vector-issue slots incl. two transcendentals), at ~5
// slots + one 2-byte LDS gather.  Arguments outside the table (|x| < 6.1e-5: probability ~5e-5; |x| >= 16) make the
// caller fall back to the formula for that group of values (wave-uniform branch).
// ------------------------------------------------------------------------------------------------
constexpr int GT_LO = (127 - 14) << 7;       // bf16 bits of 2^-14
constexpr int GT_HALF = 18 * 128;            // entries per sign
constexpr int GT_N = 2 * GT_HALF;
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

// entry i <-> bf16 bits ((i / GT_HALF) << 15) | (GT_LO + i % GT_HALF)
__device__ __forceinline__ uint16_t gelu_tab_arg(int i) { return (uint16_t)(((i / GT_HALF) << 15) | (GT_LO + i % GT_HALF)); }

// two packed bf16 arguments -> byte offsets (packed u16 pair) into a table of `ESZ`-byte entries; `bad` is set when either
// argument is outside the table (the offsets are then clamped and the caller must not use the looked-up values).  SIGNED = false: a
// table that holds the POSITIVE arguments only (GT_HALF entries), offsets of |x|; the caller applies the sign symmetry
template <int ESZ, bool SIGNED = true>
__device__ __forceinline__ uint32_t gelu_tab_off2(uint32_t w, bool& bad) {
    const u16x2_t a = __builtin_bit_cast(u16x2_t, w & 0x7fff7fffu);
    const u16x2_t lo = {(unsigned short)GT_LO, (unsigned short)GT_LO};
    const u16x2_t mx = {(unsigned short)(GT_HALF - 1), (unsigned short)(GT_HALF - 1)};
    const u16x2_t idx = a - lo;                                      // wraps for arguments below the table
    const u16x2_t idc = __builtin_elementwise_min(idx, mx);
    bad = bad || (__builtin_bit_cast(uint32_t, idx) != __builtin_bit_cast(uint32_t, idc));
    if constexpr (!SIGNED) return __builtin_bit_cast(uint32_t, (u16x2_t)(idc * (unsigned short)ESZ));
    const u16x2_t sg = __builtin_bit_cast(u16x2_t, w) >> 15;         // 0 / 1 per half
    const u16x2_t half = {(unsigned short)GT_HALF, (unsigned short)GT_HALF};
    const u16x2_t off = (idc + sg * half) * (unsigned short)ESZ;
    return __builtin_bit_cast(uint32_t, off);
}

// ------------------------------------------------------------------------------------------------
// The head-major window layout [Bw][h][S][Lp][DP], the contract between the engine and every attention kernel, stated once:
//   logical row m = bw * Lp + t (window, token; tokens t >= L are padding), logical column k = DP * (h * part + hd) + j
//   (S parts: 3 for q | k | v, 1 for oh; head dim padded to DP in {16, 32, 64, 96, 128}, or exactly 256; the matching weights are
//   padded by swv2_prep_weight), rnorm (1 / |q|, 1 / |k|) = [Bw][h][2][Lp].
// HeadLayout is a view: the host computes it once per operand (head_layout) and stores its magics in the descriptor of the loader or
// the epilogue (put_head_magics); the device rebuilds it from there (ALoad<A_HEADS>::lay, epi_layout).  A view built from compile-time
// values folds to constants.  heads_item / heads_item_wide (gemm_epilogue.h) and the loader's split keep their own text of the two
// splits: through this struct they compile to other instruction streams (LABNOTES, "Forward GEMM engine by role").
// ------------------------------------------------------------------------------------------------
constexpr bool head_pad_ok(int dp) { return dp == 16 || dp == 32 || dp == 64 || dp == 96 || dp == 128 || dp == 256; }
constexpr int head_pad_log2(int dp) { return dp == 16 ? 4 : dp == 32 ? 5 : dp == 64 ? 6 : dp == 128 ? 7 : dp == 256 ? 8 : -1; }   // -1: no power of two

struct HeadLayout {
    int h, S, Lp, DP;
    uint32_t mg_lp, mg_h, mg_dp;        // fdiv magics of Lp, h, DP
    struct Row { int bw, t; };
    struct Col { int part, hd, j; };
    __device__ __forceinline__ Row row(int m) const {
        const int bw = fdiv(m, Lp, mg_lp);
        return {bw, m - bw * Lp};
    }
    // ph = k / DP, however the caller divided (a compile-time DP, a shift)
    __device__ __forceinline__ Col col_of(int ph, int k) const {
        const int j = k - ph * DP, part = (h == 1) ? ph : fdiv(ph, h, mg_h);
        return {part, ph - part * h, j};
    }
    // element offset of channel 0 of (bw, hd, part, t) -- channel j is + j, which the callers add to the pointer themselves (address =
    // base + row offset + channel); the 32-bit form for callers that checked the tensor against 2^32 bytes
    __device__ __forceinline__ long off(int bw, int hd, int part, int t) const { return ((((long)bw * h + hd) * S + part) * Lp + t) * DP; }
    __device__ __forceinline__ uint32_t off32(int bw, int hd, int part, int t) const { return (uint32_t)((((bw * h + hd) * S + part) * Lp + t) * DP); }
    __device__ __forceinline__ long rnorm_off(int bw, int hd, int part, int t) const { return (((long)bw * h + hd) * 2 + part) * Lp + t; }
};
static inline HeadLayout head_layout(int h, int S, int Lp, int DP) {
    return {h, S, Lp, DP, fdiv_magic(Lp), fdiv_magic(h), fdiv_magic(DP)};
}
template <class Desc> void put_head_magics(Desc& d, const HeadLayout& l) { d.mg0 = l.mg_lp; d.mg1 = l.mg_h; d.mg2 = l.mg_dp; }

// ------------------------------------------------------------------------------------------------
// A loaders: chunk(m, k0) returns 8 bf16 (k0 multiple of 8) of logical row m; zeros outside [0,M)x[0,K)
// ------------------------------------------------------------------------------------------------
struct LoadDesc {           // plain-data description shared by all loader kinds (filled by the host)
    const void* ptr;        // primary source
    const int32_t* rowidx;  // optional gather table: logical row -> source row, <0 = zero row
    const float* aux0;      // LN-on-load: mean[M] ; patch: unused
    const float* aux1;      // LN-on-load: rstd[M]
    const float* aux2;      // LN-on-load: gamma[K]
    const float* aux3;      // LN-on-load: beta[K]
    long ld;                // source row pitch in elements
    int M, K;
    int p0, p1, p2, p3;     // kind-specific ints (see loaders)
    uint32_t mg0, mg1, mg2; // fdiv magics of the kind-specific divisors (make_loader)
};

template <int KIND> struct ALoad;

enum { A_F32 = 0, A_BF16 = 1, A_BF16_GELU = 2, A_HEADS = 3, A_PATCH = 4, A_MERGE_LN = 5, A_BF16_CS = 6 };

struct RawF32 { f32x4 a, b; };
__device__ __forceinline__ uint4 cvt_f32x8(const RawF32& r) {
    uint4 o;
    o.x = f2bf2(r.a[0], r.a[1]); o.y = f2bf2(r.a[2], r.a[3]); o.z = f2bf2(r.b[0], r.b[1]); o.w = f2bf2(r.b[2], r.b[3]);
    return o;
}
__device__ __forceinline__ RawF32 ld_f32x8(const float* p) {
    RawF32 o = {*(const f32x4*)p, *(const f32x4*)(p + 4)};
    return o;
}

// Every loader has two phases: raw() issues the global loads and returns the registers untouched, cvt() produces the
// 8 bf16.  The conversion happens when the tile is written to LDS, so the loads stay in flight across the MFMA phase
// (a loader that converts inside the load makes the compiler wait for the data right there).  chunk() = cvt(raw()).
// A kind states its Raw type, raw_unc, cvt, its flags and (LINEAR kinds) raw_lin; the base derives the rest:
//   raw_unc(r, k0)  UNCONDITIONAL load of source row r in [0, rows), k0 in [0, K): no exec-masked load, so the compiler can count it
//                   in s_waitcnt and a prefetch stays in flight (a load under `if` makes it guard the destination with vmcnt(0))
//   raw_lin(off)    LINEAR: element offset (row * ld + k0, below 2^32: checked by the launchers) -> unconditional load, scalar
//                   base + 32-bit offset
//   row_of(m)       source row of logical row m, -1 = a zero row (m >= M, a negative gather entry): ONE dependent load for GATHER
//                   kinds, hoisted by the kernels
//   raw_at(r, k0)   zeros for a zero row or k0 >= K, else raw_unc.  The zero-row test has two spellings, r < 0 and (ROW_PAST_M) "r < 0
//                   stands for row M, rows >= M are zero": one rule, but they compile to different instruction streams inside the
//                   kernels' k-loops, and each kind keeps the one it was tuned and measured with
template <class L, class RawT> struct ALoadBase {
    static constexpr bool ROW_FASTEST = false;      // staging thread map: adjacent threads take adjacent rows (not adjacent chunks of a row)
    static constexpr bool LINEAR = false;           // un-gathered rows are ptr + row * ld: the kernels may form the offsets incrementally
    static constexpr bool GATHER = false;           // rows go through d.rowidx where the operand has one
    static constexpr bool ROW_PAST_M = true;        // raw_at's spelling of the zero-row test (above)
    typedef RawT Raw;
    LoadDesc d;
    // the chunk of a zero row.  (HEADS and MERGE_LN spell the same value make_uint4(0, 0, 0, 0), as they always have: like
    // ROW_PAST_M, the spelling moves the instruction streams of the kernels' k-loops)
    static __device__ __forceinline__ Raw zero() { return Raw{}; }
    // the operand as bf16 (the raw bf16 kinds)
    __device__ __forceinline__ const uint16_t* bf() const { return (const uint16_t*)d.ptr; }
    __device__ __forceinline__ int row_of(int m) const {
        if (m >= d.M) return -1;
        if constexpr (L::GATHER) { if (d.rowidx) return d.rowidx[m]; }
        return m;
    }
    __device__ __forceinline__ Raw raw_at(int r, int k0) const {
        if constexpr (L::ROW_PAST_M) {
            const int m = r < 0 ? d.M : r;
            if (m >= d.M || k0 >= d.K) return L::zero();
            return static_cast<const L*>(this)->raw_unc(m, k0);
        } else {
            if (r < 0 || k0 >= d.K) return L::zero();
            return static_cast<const L*>(this)->raw_unc(r, k0);
        }
    }
    __device__ __forceinline__ Raw raw(int m, int k0) const { return raw_at(row_of(m), k0); }
    __device__ __forceinline__ uint4 chunk(int m, int k0) const { return static_cast<const L*>(this)->cvt(raw(m, k0)); }
};

// fp32 rows (optionally gathered): the residual stream x[B*T][C]
template <> struct ALoad<A_F32> : ALoadBase<ALoad<A_F32>, RawF32> {
    static constexpr bool LINEAR = true, GATHER = true, ROW_PAST_M = false;
    __device__ __forceinline__ Raw raw_lin(uint32_t off) const { return ld_f32x8((const float*)d.ptr + off); }
    __device__ __forceinline__ Raw raw_unc(int r, int k0) const { return ld_f32x8((const float*)d.ptr + (long)r * d.ld + k0); }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const { return cvt_f32x8(r); }
};
// bf16 rows (optionally gathered)
template <> struct ALoad<A_BF16> : ALoadBase<ALoad<A_BF16>, uint4> {
    static constexpr bool LINEAR = true, GATHER = true, ROW_PAST_M = false;
    __device__ __forceinline__ Raw raw_lin(uint32_t off) const { return *(const uint4*)(bf() + off); }
    __device__ __forceinline__ Raw raw_unc(int r, int k0) const { return *(const uint4*)(bf() + (long)r * d.ld + k0); }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const { return r; }
};
// bf16 rows scaled on load by an fp32 factor per (sample, 16-column group): the head's loss-gradient operand
//   G[m][n] = coef[b(m)][n / 16] * R[m][n],  R = quadrature-weighted residual written by the un-patchify + loss epilogue
// p0 = rows per sample (mg0 its magic), p2 = groups per sample in aux0.  The factor is loaded with the data (raw), applied
// when the tile is written to LDS (cvt).
struct RawCS { uint4 v; float s; };
template <> struct ALoad<A_BF16_CS> : ALoadBase<ALoad<A_BF16_CS>, RawCS> {
    static constexpr bool ROW_PAST_M = false;
    __device__ __forceinline__ Raw raw_unc(int r, int k0) const {
        const int b = fdiv(r, d.p0, d.mg0);
        Raw o = {*(const uint4*)(bf() + (long)r * d.ld + k0), d.aux0[b * d.p2 + (k0 >> 4)]};
        return o;
    }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const {
        float v[8];
        unpack8(r.v, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= r.s;
        return pack8(v);
    }
};
// bf16 rows through GELU (fc2 input = GELU(fc1 output); the pre-activation is what is kept for backward)
template <> struct ALoad<A_BF16_GELU> : ALoadBase<ALoad<A_BF16_GELU>, uint4> {
    static constexpr bool LINEAR = true;
    const uint16_t* tab = nullptr;      // LDS table of bf16(GELU(x)) (see gelu_tab_off2), set by the kernel; null = formula
    __device__ __forceinline__ Raw raw_lin(uint32_t off) const { return *(const uint4*)(bf() + off); }
    __device__ __forceinline__ Raw raw_unc(int r, int k0) const { return *(const uint4*)(bf() + (long)r * d.ld + k0); }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const {
        if (tab) {
            bool bad = false;
            const uint32_t o[4] = {gelu_tab_off2<2>(r.x, bad), gelu_tab_off2<2>(r.y, bad), gelu_tab_off2<2>(r.z, bad),
                                   gelu_tab_off2<2>(r.w, bad)};
            if (!__builtin_expect(__any((int)bad), 0)) {
                const unsigned char* tb = (const unsigned char*)tab;
                uint32_t q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    q[i] = (uint32_t)*(const uint16_t*)(tb + (o[i] & 0xffffu)) | ((uint32_t)*(const uint16_t*)(tb + (o[i] >> 16)) << 16);
                return make_uint4(q[0], q[1], q[2], q[3]);
            }
        }
        float v[8];
        unpack8(r, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = gelu_f(v[i]);
        return pack8(v);
    }
};
// the head-major window layout (HeadLayout): p0 = heads, p1 = log2(DP) or -1, p2 = Lp, p3 = DP, ld = number of parts S (1 for oh,
// 3 for dqkvh), mg0 .. mg2 = the layout's magics (make_loader)
template <> struct ALoad<A_HEADS> : ALoadBase<ALoad<A_HEADS>, uint4> {
    static __device__ __forceinline__ Raw zero() { return make_uint4(0, 0, 0, 0); }
    __device__ __forceinline__ HeadLayout lay() const { return {d.p0, (int)d.ld, d.p2, d.p3, d.mg0, d.mg1, d.mg2}; }
    // (row m, column k0) -> window, token, part, head, channel; p1 picks the shift
    struct Split { int bw, t, part, hd, j; };
    __device__ __forceinline__ Split split(int m, int k0) const {
        const int h = d.p0, Lp = d.p2, DP = d.p3;
        const int bw = fdiv(m, Lp, d.mg0), t = m - bw * Lp;
        const int ph = d.p1 >= 0 ? (k0 >> d.p1) : fdiv(k0, DP, d.mg2), j = k0 - ph * DP;
        const int part = (h == 1) ? ph : fdiv(ph, h, d.mg1), hd = ph - part * h;
        return {bw, t, part, hd, j};
    }
    __device__ __forceinline__ Raw raw_unc(int m, int k0) const {
        const Split s = split(m, k0);
        return *(const uint4*)(bf() + lay().off(s.bw, s.hd, s.part, s.t) + s.j);
    }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const { return r; }
    // element offset of (row m, column k0) for callers that address with 32 bits (tensor below 2^32 bytes, checked by them)
    __device__ __forceinline__ uint32_t elem_off(int m, int k0) const {
        const Split s = split(m, k0);
        return lay().off32(s.bw, s.hd, s.part, s.t) + (uint32_t)s.j;
    }
    // Walking rows m, m + 16, m + 32, ... of ONE chunk column (the weight-gradient kernel's staging): the window / token split
    // once per step (step_base), then adds -- a row block that runs past its window's Lp rows continues (h S - 1) Lp DP
    // elements further, in the same (head, part) slab of the next window.  Valid while a step spans at most one window
    // boundary (16 * chunks <= Lp, checked by the caller); 32-bit element offsets.
    struct Step { uint32_t off0; int t0; };
    __device__ __forceinline__ Step step_base(int m, int k0) const {
        const Split s = split(m, k0);
        Step o = {lay().off32(s.bw, s.hd, s.part, s.t) + (uint32_t)s.j, s.t};
        return o;
    }
    __device__ __forceinline__ uint32_t step_off(const Step& b, int i) const {
        const int Lp = d.p2, DP = d.p3;
        const uint32_t hop = (uint32_t)((d.p0 * (int)d.ld - 1) * Lp * DP);
        return b.off0 + (uint32_t)(16 * i * DP) + ((b.t0 + 16 * i >= Lp) ? hop : 0u);
    }
    __device__ __forceinline__ Raw raw_lin(uint32_t off) const { return *(const uint4*)(bf() + off); }
};
// PatchEmbed im2col: x[B][Cin][H][W] fp32, row m = (b, i, j) patch, k = cin*16 + p*4 + q (conv weight order)
// p0 = Cin, p1 = H, p2 = W ; patch = 4.  Adjacent rows are adjacent 16-byte groups -> row-fastest thread map.
template <> struct ALoad<A_PATCH> : ALoadBase<ALoad<A_PATCH>, RawF32> {
    static constexpr bool ROW_FASTEST = true;
    __device__ __forceinline__ Raw raw_unc(int m, int k0) const {
        const int Cin = d.p0, H = d.p1, W = d.p2, gw = W >> 2, gh = H >> 2;
        const int b = fdiv(m, gh * gw, d.mg0), ij = m - b * gh * gw, i = fdiv(ij, gw, d.mg1), j = ij - i * gw;
        const int cin = k0 >> 4, p = (k0 >> 2) & 3;                 // p in {0, 2}
        // p3 = channels per sample of the tensor that holds the Cin planes (0 = Cin: a dense [B][Cin][H][W] tensor); the
        // rollout's step outputs are channel slices of one [B][(n_future+1) Cout][H][W] buffer
        const int Ct = d.p3 ? d.p3 : Cin;
        const float* src = (const float*)d.ptr + (((long)b * Ct + cin) * H + 4 * i + p) * W + 4 * j;
        Raw o = {*(const f32x4*)src, *(const f32x4*)(src + W)};
        if (d.aux0) {   // second source added on load (ld = its channels per sample): gradient of the fed-back prediction
            const float* s2 = d.aux0 + (((long)b * d.ld + cin) * H + 4 * i + p) * W + 4 * j;
            o.a += *(const f32x4*)s2;
            o.b += *(const f32x4*)(s2 + W);
        }
        return o;
    }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const { return cvt_f32x8(r); }
};
// PatchMerging gather + LayerNorm(4C) on load: x[B][H][W][C] fp32, row m = (b, i, j) on the half grid,
// k = (wp*2 + hp)*C + c  (swinv2_global.py:520) ; p0 = H, p1 = W, p2 = C ; aux = mean, rstd, gamma, beta
template <> struct ALoad<A_MERGE_LN> : ALoadBase<ALoad<A_MERGE_LN>, uint4> {
    static __device__ __forceinline__ Raw zero() { return make_uint4(0, 0, 0, 0); }
    __device__ __forceinline__ Raw raw_unc(int m, int k0) const {
        const int H = d.p0, W = d.p1, C = d.p2, h2 = H >> 1, w2 = W >> 1;
        const int b = m / (h2 * w2), ij = m - b * h2 * w2, i = ij / w2, j = ij - i * w2;
        const float mu = d.aux0[m], rs = d.aux1[m];
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e, blk = k / C, c = k - blk * C, wp = blk >> 1, hp = blk & 1;
            const float x = ((const float*)d.ptr)[(((long)b * H + 2 * i + hp) * W + 2 * j + wp) * C + c];
            v[e] = (x - mu) * rs * d.aux2[k] + d.aux3[k];
        }
        return pack8(v);
    }
    __device__ __forceinline__ uint4 cvt(const Raw& r) const { return r; }
};

// ------------------------------------------------------------------------------------------------
// The destination rule of every weight gradient, stated once (swv2.h, swv2_linear_wgrad): output row n goes to nmap[n], column k to
// kmap[k] (no map: itself); a negative entry drops the element; what is kept accumulates onto dW[n][k] (row pitch ldw) / db[n].
// wg_index: one index through its optional map; the caller keeps the element where every mapped index is >= 0.  Used by the epilogue
// of tn_tile (dW and db), by tn_reduce_kernel and by the bias part of tn_wide_reduce_kernel.  The dW part of tn_wide_reduce_kernel and
// both parts of tn_slab_reduce_kernel keep the same expression open-coded: through this helper they compile to another branch
// structure, and so does every site through a helper that returns the address or a "keep" flag (LABNOTES "Weight-gradient engine by
// role").
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wg_index(const int32_t* map, int i) { return map ? map[i] : i; }

template <int AK>
ALoad<AK> make_loader(const swv2_operand* o) {
    ALoad<AK> l;
    l.d.ptr = o->ptr; l.d.rowidx = o->rowidx; l.d.aux0 = o->aux0; l.d.aux1 = o->aux1; l.d.aux2 = o->aux2;
    l.d.aux3 = o->aux3; l.d.ld = o->ld; l.d.M = o->rows; l.d.K = o->cols;
    l.d.p0 = o->p[0]; l.d.p1 = o->p[1]; l.d.p2 = o->p[2]; l.d.p3 = o->p[3];
    l.d.mg0 = l.d.mg1 = l.d.mg2 = 0;
    if (AK == A_HEADS) {
        l.d.p1 = head_pad_log2(o->p[3]);
        put_head_magics(l.d, head_layout(o->p[0], (int)o->ld, o->p[2], o->p[3]));
    }
    if (AK == A_PATCH) { l.d.mg0 = fdiv_magic((o->p[1] / 4) * (o->p[2] / 4)); l.d.mg1 = fdiv_magic(o->p[2] / 4); }
    if (AK == A_BF16_CS) l.d.mg0 = fdiv_magic(o->p[0]);
    return l;
}

int check_operand(const swv2_operand* o, const char* who) {
    SWV2_CHECK_ARG(o && o->ptr, "%s: null operand", who);
    SWV2_CHECK_ARG(o->rows > 0 && o->cols > 0, "%s: empty operand", who);
    SWV2_CHECK_ARG(o->cols % 8 == 0, "%s: operand width %d must be a multiple of 8", who, o->cols);
    SWV2_CHECK_ARG(((uintptr_t)o->ptr & 15) == 0, "%s: operand pointer must be 16-byte aligned", who);
    if (o->kind == SWV2_OP_F32 || o->kind == SWV2_OP_BF16 || o->kind == SWV2_OP_BF16_GELU || o->kind == SWV2_OP_BF16_CSCALE)
        SWV2_CHECK_ARG(o->ld % 8 == 0 && o->ld >= o->cols, "%s: row pitch %ld must be a multiple of 8 and >= cols", who, o->ld);
    if (o->kind == SWV2_OP_F32 || o->kind == SWV2_OP_BF16 || o->kind == SWV2_OP_BF16_GELU)
        SWV2_CHECK_ARG((double)o->rows * (double)o->ld < 4.29e9, "%s: row-major operands are indexed with 32-bit element offsets (%d x %ld too large)", who, o->rows, o->ld);
    if (o->kind == SWV2_OP_BF16_CSCALE)
        SWV2_CHECK_ARG(o->aux0 && o->p[0] > 0 && o->p[2] * 16 >= o->cols && o->cols % 16 == 0 && !o->rowidx,
                       "%s: scaled operand needs aux0, rows per sample p[0] > 0, p[2] >= cols / 16 groups, no gather", who);
    if (o->kind == SWV2_OP_HEADS)
        SWV2_CHECK_ARG(head_pad_ok(o->p[3]), "%s: head pad %d not in {16,32,64,96,128,256}", who, o->p[3]);
    if (o->kind == SWV2_OP_PATCH)
        SWV2_CHECK_ARG(o->p[1] % 4 == 0 && o->p[2] % 4 == 0 && o->cols == o->p[0] * 16, "%s: bad patch geometry", who);
    if (o->kind == SWV2_OP_MERGE_LN)
        SWV2_CHECK_ARG(o->aux0 && o->aux1 && o->aux2 && o->aux3 && o->cols == 4 * o->p[2], "%s: bad merge operand", who);
    return SWV2_OK;
}

}  // namespace
