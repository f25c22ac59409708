// The 256 x 256 NT kernels of the GEMM engine (LinearKernel::WIDE_DMA, LinearKernel::WIDE; chosen by linear_kernel_for in gemm.hip,
// launched through swv2_nt_wide_launch below).  Loaders: gemm_common.h; the wave-tile epilogue (wide_epilogue): gemm_epilogue.h.
#include "common.h"

#include "gemm_epilogue.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Wide NT kernel: 256 x 256 x 64 tiles for the MFMA-bound products of wide models (the reference's own swin_73var is
// embed_dim 768: K and N of 768 .. 3072, where gemm_nt_kernel's 64 x 64 wave tiles and its single LDS buffer with two
// barriers per k-step reach 8 - 23 % of the matrix peak).  One 8-wave workgroup per CU, wave tile 128 x 64 (128 fp32
// accumulators; per K = 32: 12 ds_read_b128 for 32 MFMAs), two LDS tile buffers (2 x 64 KB) with the next k-step's global
// loads in flight in registers across the MFMAs and ONE barrier per k-step.  All staging loads are unconditional (rows
// past M: the operand's first row, zeroed at commit), so the compiler can count them in s_waitcnt.
// Grid: one workgroup per output tile.  Workgroups are dispatched round-robin over the 8 XCDs (blockIdx % 8), each XCD
// with its own L2; the index is decoded so that the ~32 tiles an XCD runs concurrently are 8 row panels x 4 column tiles:
// every A line is then fetched from HBM / Infinity Cache once per 4 and every weight line once per 8 workgroups instead of
// once each (speed only: any mapping is correct).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz32(int r, int c) { return r * 32 + ((c ^ ((0 - (r >> 2)) & 3)) << 3); }

// decode the v-th tile of XCD x (see the header comment): false = past the matrix
__device__ __forceinline__ bool wide_tile(int x, int v, int mtiles, int ntn, int& mt, int& nt) {
    const int per_group = 8 * ntn;
    const int gl = v / per_group, r = v - gl * per_group;
    const int nb = r >> 5, rr = r & 31;               // column block of 4 tiles; (panel, column) inside it: rr < 8 * min(4, ntn - 4 nb)
    mt = (gl * 8 + x) * 8 + (rr & 7);
    nt = 4 * nb + (rr >> 3);
    return mt < mtiles && nt < ntn;
}

// ---- raw bf16 operands (A_BF16 without a gather table, A_HEADS): both operands reach LDS by DMA, no staging registers ----
// Persistent workgroups (32 per XCD) walk their XCD's tile sequence; the DMA pipeline runs THROUGH the tile boundaries.
//   LDS: four stage slots of 32 k (A[256][32] | B[256][32] bf16 = 32 KB each; 64-byte rows, chunk c of row r at physical chunk
//   c ^ ((-(r >> 2)) & 3): the 16 lanes ds_read_b128 serves per cycle ({0-3, 12-15, 20-27}, ...) then fall on 16 different 16-byte
//   bank groups) + a 2 KB pad behind slot 3 (the epilogue's staging = slot 3 + pad).  Global stage q = (tile, 32-k step) lives in
//   slot q & 3; K is a multiple of 128, so a tile's last stage sits in slot 3 and the next tile's stages 0, 1, 2 -- issued during
//   the last three steps of this tile -- in slots 0, 1, 2.
// Two wave groups (waves 0-3: rows 0-127 of the tile, waves 4-7: rows 128-255; waves w and w + 4 share a SIMD) run the same loop
// one barrier apart: while one group issues its 32 MFMAs of a stage, the other issues DMA and reads its fragments from LDS, so
// each SIMD's matrix pipe always has one wave feeding it.  Per stage t and wave:
//     LOAD(t): 4 DMA instructions of stage t + 3 -> slot (t + 3) & 3 | 12 ds_read_b128 of stage t | vmcnt(8) | lgkmcnt(0)
//     barrier | MFMA(t): 32 MFMAs | barrier
// group 0 runs LOAD(t) in section 2 t and MFMA(t) in section 2 t + 1, group 1 one section later (sections = the intervals between
// workgroup barriers).  RAW: a wave retires its own DMA of stage t + 1 with the counted vmcnt(8) at the end of LOAD(t) (stages
// t + 2, t + 3 = 8 instructions stay in flight; VMEM operations retire in order, so older epilogue stores only make the wait
// longer), i.e. by the end of section 2 t + 1 at the latest; the first read of stage t + 1 is in section 2 t + 2, behind that
// section's opening barrier.  WAR: slot (t + 3) & 3 held stage t - 1, whose last reads (group 1, LOAD(t - 1), retired by its
// lgkmcnt(0)) are in section 2 t - 1; the DMA into it is issued in sections 2 t (group 0) and 2 t + 1 (group 1).  Every wave issues
// exactly 4 DMA instructions per stage, in stage order; behind the last tile the last stage is re-read into slots nobody reads.
// Tile end (last stage L in slot 3): group 0 waits one section, BOTH groups run the epilogue in the same section (staging in
// slot 3 + pad: the last reads of slot 3 are two sections back, the next DMA into it is issued in LOAD(0) of the next tile, one
// barrier later), then group 1 waits one section: the stagger is restored.  Two idle sections per tile buy the epilogues of all
// eight waves side by side and a prologue that is already in LDS.
template <int AK, int EK>
__global__ __launch_bounds__(WTH) void gemm_nt_wide_dma_kernel(ALoad<AK> al, const uint16_t* __restrict__ Wb, Epi<EK> ep,
                                                               int M, int N, int K, int mtiles, int ntn, int vmax) {
    static_assert(AK == A_BF16 || AK == A_HEADS, "DMA needs a raw bf16 operand");
    __shared__ __attribute__((aligned(1024))) unsigned char smem_b[WSM_BYTES];
    static_assert(3 * WSTG * 2 + 8 * 16 * EP * 4 <= WSM_BYTES, "epilogue staging = slot 3 + pad");
    uint16_t* const smem = (uint16_t*)smem_b;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int wr = wave >> 2, wc = wave & 3;              // 2 x 4 waves, 128 x 64 each
    const int xcd = blockIdx.x & 7, nper = gridDim.x >> 3, stages = K / 32;
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    // DMA geometry: one wave instruction fills 16 stage rows x 64 bytes (1 KB of LDS); instruction i (of 2 per operand) of this
    // wave covers rows 32 wave + 16 i .. + 15; lane -> (row + (lane >> 2), physical chunk lane & 3)
    const int drow = wave * 32 + (lane >> 2);
    int dkc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) dkc[i] = (lane & 3) ^ ((0 - ((drow + 16 * i) >> 2)) & 3);
    struct Tile { int m_base, n_base; uint32_t boff[2], aoff[2]; };
    auto make_tile = [&](int mt, int nt) {
        Tile t;
        t.m_base = mt * WBM; t.n_base = nt * WBN;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = drow + 16 * i;
            t.boff[i] = 2u * (uint32_t)(min(t.n_base + row, N - 1) * K + dkc[i] * 8);      // (N = 192, one partial column tile: rows past N re-read the last one, their columns are never stored)
            t.aoff[i] = AK == A_BF16 ? 2u * (uint32_t)(min(t.m_base + row, M - 1) * (int)al.d.ld + dkc[i] * 8) : 0u;
        }
        return t;
    };
    auto issue = [&](const Tile& tl, int t, int slot) {
        const uint32_t la = lds0 + (uint32_t)(slot * WSTG * 2) + (uint32_t)(wave * 2048), lb = la + WBM * 32 * 2;
#pragma unroll
        for (int i = 0; i < 2; ++i) dma_x4(Wb + t * 32, tl.boff[i], lb + 1024 * i);
        if constexpr (AK == A_BF16) {
#pragma unroll
            for (int i = 0; i < 2; ++i) dma_x4((const uint16_t*)al.d.ptr + t * 32, tl.aoff[i], la + 1024 * i);
        } else {                             // head-major rows: the element offset of (row, k) is not affine in k
#pragma unroll
            for (int i = 0; i < 2; ++i)
                dma_x4(al.d.ptr, 2u * al.elem_off(min(tl.m_base + drow + 16 * i, M - 1), t * 32 + dkc[i] * 8), la + 1024 * i);
        }
    };
    // first tile of this workgroup
    int v = blockIdx.x >> 3, mt = 0, nt = 0;
    while (v < vmax && !wide_tile(xcd, v, mtiles, ntn, mt, nt)) v += nper;
    if (v >= vmax) return;
    Tile cur = make_tile(mt, nt);
    issue(cur, 0, 0); issue(cur, 1, 1); issue(cur, 2, 2);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");       // stage 0 has landed (this wave's part)
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();             // group 1 starts one section later
    for (;;) {
        int v2 = v + nper, mt2 = 0, nt2 = 0;
        while (v2 < vmax && !wide_tile(xcd, v2, mtiles, ntn, mt2, nt2)) v2 += nper;
        const bool has_next = v2 < vmax;
        const Tile nxt = has_next ? make_tile(mt2, nt2) : cur;
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < stages; ++t) {
            // ---- LOAD(t)
            if (t + 3 < stages) issue(cur, t + 3, (t + 3) & 3);
            else issue(nxt, has_next ? t + 3 - stages : stages - 1, (t + 3) & 3);
            const uint16_t* As = smem + (t & 3) * WSTG;
            const uint16_t* Bs = As + WBM * 32;
            bf16x8 af[8], bf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const bf16x8*)(Bs + swz32(wc * 64 + j * 16 + fr, g));
#pragma unroll
            for (int i = 0; i < 8; ++i) af[i] = *(const bf16x8*)(As + swz32(wr * 128 + i * 16 + fr, g));
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            // ---- MFMA(t)
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- tile end
        if (wr == 0) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        {
            float* st = (float*)(smem + 3 * WSTG) + wave * 16 * EP;
            if (cur.n_base + wc * 64 < N) wide_epilogue<EK>(ep, acc, st, cur.m_base + wr * 128, cur.n_base + wc * 64, lane);      // (N: a multiple of 64)
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the staging reads are done before slot 3 is handed back
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        if (wr == 1) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (!has_next) break;
        cur = nxt; v = v2;
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();             // (every wave passes the same number of barriers)
}

// ---- register-staged A (fp32 rows, gathered rows with zero rows): weights by DMA, two 64-k buffers, one tile per workgroup ----
template <int AK, int EK>
__global__ __launch_bounds__(WTH) void gemm_nt_wide_kernel(ALoad<AK> al, const uint16_t* __restrict__ Wb, Epi<EK> ep,
                                                           int M, int N, int K, int mtiles, int ntn) {
    static_assert(!ALoad<AK>::ROW_FASTEST, "row-major staging map only");
    constexpr int TILE = (WBM + WBN) * BK;                 // elements per 64-k buffer (A | B)
    __shared__ __attribute__((aligned(1024))) uint16_t smem[2 * TILE];
    static_assert(2 * TILE * 2 >= 8 * 16 * EP * 4, "the epilogue staging re-uses the tile buffers");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int wr = wave >> 2, wc = wave & 3;              // 2 x 4 waves, 128 x 64 each
    int mt, nt;
    if (!wide_tile(blockIdx.x & 7, blockIdx.x >> 3, mtiles, ntn, mt, nt)) return;
    const int m_base = mt * WBM, n_base = nt * WBN;
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const int ksteps = K / BK;
        // DMA geometry (weights): one wave instruction fills 8 tile rows x 128 bytes; instruction i of this wave covers tile
        // rows 32 wave + 8 i .. + 7; lane -> (row + (lane >> 3), physical chunk lane & 7), which holds logical chunk (lane & 7) ^ swizzle
        // (= swz_chunk(row, lane & 7), spelled out: through the helper this kernel's register counts change)
        const int drow = wave * 32 + (lane >> 3);
        uint32_t boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = drow + 8 * i, kcl = (lane & 7) ^ ((row >> 1) & 7);
            boff[i] = 2u * (uint32_t)((n_base + row) * K + kcl * 8);
        }
        // register staging of A: 4 chunks of 16 bytes per thread per k-step; chunk c = tid + 512 i -> (row c >> 3, chunk column c & 7)
        typename ALoad<AK>::Raw ra[4];
        int arow[4];
        uint32_t aok = 0;
        const int kc = tid & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int src = al.row_of(m_base + (tid >> 3) + 64 * i);
            arow[i] = max(src, 0);
            aok |= (src >= 0 ? 1u : 0u) << i;
        }
        auto issue = [&](int s, int buf) {
            const uint32_t lb = lds0 + (uint32_t)(buf * TILE * 2) + (uint32_t)(wave * 4096) + WBM * BK * 2;
#pragma unroll
            for (int i = 0; i < 4; ++i) dma_x4(Wb + s * BK, boff[i], lb + 1024 * i);
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i] = al.raw_unc(arow[i], s * BK + kc * 8);
        };
        auto commit = [&](int buf) {
            uint16_t* As = smem + buf * TILE;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint4 v = al.cvt(ra[i]);
                if (!((aok >> i) & 1)) v = make_uint4(0, 0, 0, 0);
                *(uint4*)(As + swz((tid >> 3) + 64 * i, kc)) = v;
            }
        };
        auto compute = [&](int buf) {
            const uint16_t* As = smem + buf * TILE;
            const uint16_t* Bs = As + WBM * BK;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 bf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = *(const bf16x8*)(Bs + swz(wc * 64 + j * 16 + fr, kk * 4 + g));
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const bf16x8 af = *(const bf16x8*)(As + swz(wr * 128 + i * 16 + fr, kk * 4 + g));
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma32(af, bf[j], acc[i][j]);
                }
            }
        };
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        commit(0);
        __syncthreads();
        for (int s = 0; s + 1 < ksteps; ++s) {
            issue(s + 1, (s + 1) & 1);
            // (without the fences the scheduler sinks the loads behind the MFMAs, next to the waits of commit, or re-issues them
            // there: found in the ISA, 7 400 cycles per k-step against 2 048 of MFMA work)
            __builtin_amdgcn_sched_barrier(0);
            compute(s & 1);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the DMA'd weight tile of step s + 1 has landed
            commit((s + 1) & 1);
            __syncthreads();           // step s + 1 is complete in its buffer; every wave is done reading buffer s & 1
        }
        compute((ksteps - 1) & 1);
        __syncthreads();               // the staging below overwrites the tile buffers
    }
    wide_epilogue<EK>(ep, acc, (float*)smem + wave * 16 * EP, m_base + wr * 128, n_base + wc * 64, lane);
}

// the launch shapes of the two kernels; `if constexpr` keeps the DMA kernel to the loaders it can fetch
template <int AK, int EK>
int launch_wide(bool dma, const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, int N, int K, hipStream_t st) {
    // 32-bit byte offsets in the DMA addressing: weights below 4 GB (the operand: part of the selection)
    SWV2_CHECK_ARG((double)N * K * 2 < 4.29e9, "swv2_linear: weight too large for the wide kernel's 32-bit offsets");
    const Epi<EK> ep = make_epi<EK>(e, M, N);
    const uint16_t* wb = (const uint16_t*)w;
    const int mtiles = cdiv(M, WBM), ntn = cdiv(N, WBN), groups = cdiv(mtiles, 8);
    const int vmax = cdiv(groups, 8) * 8 * ntn;            // tile sequence length per XCD
    if (dma) {
        // persistent: at most 32 workgroups per XCD walk the tile sequence (a grid choice, not another kernel)
        if constexpr (dma_loader(AK))
            hipLaunchKernelGGL((gemm_nt_wide_dma_kernel<AK, EK>), dim3(8 * (vmax < 32 || !swv2_wide_persist() ? vmax : 32)), dim3(WTH), 0, st,
                               make_loader<AK>(a), wb, ep, M, N, K, mtiles, ntn, vmax);
    } else {
        hipLaunchKernelGGL((gemm_nt_wide_kernel<AK, EK>), dim3(8 * vmax), dim3(WTH), 0, st, make_loader<AK>(a), wb, ep, M, N, K, mtiles, ntn);
    }
    return SWV2_OK;
}
template <int AK>
int launch_wide_a(int ek, bool dma, const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, int N, int K, hipStream_t st) {
    switch (ek) {                                          // the epilogues of a wide_pair
        case E_BF16: return launch_wide<AK, E_BF16>(dma, a, w, e, M, N, K, st);
        case E_F32: return launch_wide<AK, E_F32>(dma, a, w, e, M, N, K, st);
        case E_F32_ACC: return launch_wide<AK, E_F32_ACC>(dma, a, w, e, M, N, K, st);
        case E_QKV_HEADS: return launch_wide<AK, E_QKV_HEADS>(dma, a, w, e, M, N, K, st);
        case E_HEADS: return launch_wide<AK, E_HEADS>(dma, a, w, e, M, N, K, st);
        case E_GELU_GRAD: return launch_wide<AK, E_GELU_GRAD>(dma, a, w, e, M, N, K, st);
        case E_BF16_GELU: return launch_wide<AK, E_BF16_GELU>(dma, a, w, e, M, N, K, st);
    }
    swv2_set_error("swv2_linear: wide kernel: epilogue kind %d not instantiated", ek);
    return SWV2_ERR_UNSUPPORTED;
}

}  // namespace

// gemm.hip (launch_nt2, LinearKernel::WIDE_DMA / WIDE): the selector has checked the shape and that (ak, ek) is a wide_pair
int swv2_nt_wide_launch(int ak, int ek, bool dma, const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, int N, int K, hipStream_t st) {
    switch (ak) {
        case A_F32: return launch_wide_a<A_F32>(ek, dma, a, w, e, M, N, K, st);
        case A_BF16: return launch_wide_a<A_BF16>(ek, dma, a, w, e, M, N, K, st);
        case A_HEADS: return launch_wide_a<A_HEADS>(ek, dma, a, w, e, M, N, K, st);
    }
    swv2_set_error("swv2_linear: wide kernel: operand kind %d not instantiated", ak);
    return SWV2_ERR_UNSUPPORTED;
}
