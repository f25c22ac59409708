// bf16 MFMA GEMM engine for the tall-skinny products of the SwinV2 hot path (gfx950 / CDNA4).
//
//   NT:  C[M][N]  = A[M][K] . W[N][K]^T          forward linears, dX = dY . W  (W pre-transposed by swv2_cast_weights)
//   TN:  dW[N][K] = sum_m dY[m][N]^T . X[m][K]    weight gradients (+ bias gradient = column sums of dY)
//
// M is the token count (10^5 .. 10^6), N and K are channel counts (96 .. 1232), so every product is
// HBM-bound on the A / C streams.  The engine therefore spends its structure on the memory side:
//   * A "loader" functor maps (row, 8-element k-chunk) -> 16 bytes of bf16; it folds into the load what PyTorch does
//     as separate passes in the reference: fp32->bf16 conversion, the cyclic roll + window partition gather
//     (swinv2_global.py:457,89-101), the 4x4 patch im2col of PatchEmbed (:537), the 2x2 PatchMerging gather (:519),
//     un-merging of attention heads (:318), GELU (timm Mlp) and LayerNorm-on-load.
//   * An "epilogue" functor receives 16x64 fp32 sub-tiles staged in wave-private LDS and writes them out in
//     whatever layout the consumer wants, always as full 16-byte, row-contiguous stores: bias, the head-major
//     window-ordered q/k/v layout with the L2 normalisation of q and k (:304), GELU', un-patchify + skip (:784-802).
//   * One workgroup owns a 128-row panel of A and walks all N tiles itself, so the panel's re-reads hit its own
//     XCD's L2 instead of crossing XCDs.
// Tile: 128x128x64, 256 threads = 4 waves in a 2x2 grid of 64x64 wave tiles (16 accumulators of 16x16),
// v_mfma_f32_16x16x32_bf16, one LDS tile buffer with register-staged prefetch (issue loads for step s+1, compute
// step s, write LDS after) and 3 workgroups per CU, XOR-swizzled 128-byte LDS rows for conflict-free ds_read_b128.
//
// This file: that 128-row NT tile kernel (gemm_nt_kernel), the choice of the kernel that serves a product (LinearKernel,
// linear_kernel_for) and the entry points swv2_linear / swv2_linear_kernel.  The rest of the engine by role:
//   gemm_common.h    tile constants, swizzle, GELU, the head-major window layout, the operand loaders, host checks
//   gemm_epilogue.h  the epilogues (Epi<>, heads_item*, wide_epilogue), make_epi
//   gemm_wide.hip    the 256 x 256 NT kernels of the wide models
//   gemm_rw.hip      the resident-weight row GEMMs of a block at the benchmark width (qkv; d(qkv) -> dx)
//   gemm_tn.hip, gemm_tn_slab.hip    the weight gradients
#include "common.h"

#include <cmath>
#include <cstdlib>
#include "gemm_epilogue.h"

namespace {

// ------------------------------------------------------------------------------------------------
// NT kernel
// ------------------------------------------------------------------------------------------------
// BMT = rows per workgroup: 128 (2 x 2 waves of 64 x 64) or 64 (2 x 2 waves of 32 x 64).  The 64-row variant exists for the
// grid quantisation: at 3 workgroups per CU the chip holds 768; 1013 row tiles of 128 (local batch 2) run as 1 full + 1
// third-full round (66 % of the slots busy on average, measured 12 - 16 us of batch-independent time per launch), 2026
// tiles of 64 as 2.64 of 3 rounds.
template <int AK, int EK, int BMT = BM>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_nt_kernel(ALoad<AK> al, const uint16_t* __restrict__ Wb, Epi<EK> ep,
                                                              int M, int N, int K) {
    // one A|B tile buffer (32 KB) + wave-private epilogue staging (17 KB): 49 KB -> 3 workgroups (12 waves) per CU.
    // Latency hiding comes from the co-resident workgroups plus the register prefetch of the next step's tiles.
    // A panel: 2 k-steps resident (K <= 128: the panel is loaded and converted ONCE and reused by every N tile; PMC showed
    // the per-N-tile re-reads as real HBM traffic, 548 MB vs 330 MB algorithmic for fc1), B tile, epilogue staging.
    constexpr int ACH = BMT * KCH / NTHREADS;             // A chunks per thread per k-step (4 or 2)
    constexpr int RT = BMT / 32;                          // 16-row MFMA tiles per wave (4 or 2)
    constexpr int LOG_BMT = BMT == 128 ? 7 : 6;
    __shared__ __attribute__((aligned(16))) uint16_t smem[(2 * BMT + BN) * BK];
    __shared__ __attribute__((aligned(16))) float stage[4 * 16 * EP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;              // 2 x 2 waves, (16 RT) x 64 each
    const int m_base = blockIdx.x * BMT;
    const int ntiles = (N + BN - 1) / BN, ksteps = (K + BK - 1) / BK, steps = ntiles * ksteps;
    const bool a_res = (ksteps <= 2) && (ntiles > 1);        // A panel stays in LDS across the N tiles
    uint16_t* As0 = smem;
    uint16_t* Bs = smem + 2 * BMT * BK;

    typename ALoad<AK>::Raw ra[ACH];
    uint4 rb[4];
    // the panel rows this thread stages are the same for every (n-tile, k-step): resolve the gather ONCE
    int arow[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int c = tid + i * NTHREADS;
        arow[i] = al.row_of(m_base + (ALoad<AK>::ROW_FASTEST ? (c & (BMT - 1)) : (c >> 3)));
    }
    auto issue = [&](int s) {
        const int nt = s / ksteps, ks = s - nt * ksteps;
        const bool need_a = !a_res || nt == 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int c = tid + i * NTHREADS;
            const int kc = ALoad<AK>::ROW_FASTEST ? (c >> LOG_BMT) : (c & 7);
            if (need_a) ra[i] = al.raw_at(arow[i], ks * BK + kc * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + i * NTHREADS;
            const int rn = c >> 3, kcb = c & 7, n = nt * BN + rn, k0 = ks * BK + kcb * 8;
            rb[i] = (n < N && k0 < K) ? *(const uint4*)(Wb + (long)n * K + k0) : make_uint4(0, 0, 0, 0);
        }
    };
    auto commit = [&](int s) {
        const int nt = s / ksteps, ks = s - nt * ksteps;
        const bool need_a = !a_res || nt == 0;
        uint16_t* As = As0 + (a_res ? ks * BMT * BK : 0);
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int c = tid + i * NTHREADS;
            int r, kc;
            if (ALoad<AK>::ROW_FASTEST) { r = c & (BMT - 1); kc = c >> LOG_BMT; } else { r = c >> 3; kc = c & 7; }
            if (need_a) *(uint4*)(As + swz(r, kc)) = al.cvt(ra[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + i * NTHREADS;
            *(uint4*)(Bs + swz(c >> 3, c & 7)) = rb[i];
        }
    };

    f32x4 acc[RT][4];
    constexpr bool LOSS = EK == E_UNPATCH_LOSS || EK == E_UNPATCH_LOSS_SKIP;
    // target sets: lt[i] = this N tile's row tile i, ltn[i] = the NEXT N tile's, requested a whole N tile (two row tiles + one MFMA
    // phase) ahead: one row tile ahead the wave had 4 KB of target loads in flight -- 32 KB per CU, ~16 GB/s per CU at 2 us
    typedef typename std::conditional<LOSS, typename Epi<E_UNPATCH_LOSS>::Tar, int>::type TarT;
    [[maybe_unused]] TarT lt[RT], ltn[RT];
    [[maybe_unused]] typename std::conditional<LOSS, typename Epi<E_UNPATCH_LOSS>::Row, int>::type lrow[RT];
    if constexpr (LOSS) {
#pragma unroll
        for (int i = 0; i < RT; ++i) lrow[i] = ep.row_of(m_base + wr * 16 * RT + 16 * i, lane);
#pragma unroll
        for (int i = 0; i < RT; ++i) ep.load_tar(lrow[i], wc * 64, lt[i]);
    }
    issue(0);
    if constexpr (LOSS) commit(0);
    for (int s = 0; s < steps; ++s) {
        const int nt = s / ksteps, ks = s - nt * ksteps;
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        // LOSS: the tile of step s was committed at the end of step s - 1 -- inside the branch that ran (or did not run) the
        // epilogue, so the wait for the prefetched weight tile is a counted vmcnt(N) behind the epilogue's straight-line
        // loads / stores instead of the vmcnt(0) a wait behind the merge of the two paths gets (which would wait for every store
        // of the epilogue to complete)
        if constexpr (!LOSS) commit(s);
        __syncthreads();
        if (s + 1 < steps) issue(s + 1);
        const uint16_t* As = As0 + (a_res ? ks * BMT * BK : 0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[RT], bf[4];
#pragma unroll
            for (int i = 0; i < RT; ++i) af[i] = *(const bf16x8*)(As + swz(wr * 16 * RT + i * 16 + fr, kk * 4 + g));
#pragma unroll
            for (int i = 0; i < 4; ++i) bf[i] = *(const bf16x8*)(Bs + swz(wc * 64 + i * 16 + fr, kk * 4 + g));
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // LOSS: the transposed product (rows = output columns): see Epi<E_UNPATCH_LOSS>::tile_loss_t
                    if constexpr (LOSS) acc[i][j] = mfma32(bf[j], af[i], acc[i][j]);
                    else acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
                }
        }
        __syncthreads();                                   // tile consumed: the next commit may overwrite it
        if (ks == ksteps - 1) {
            float* st = stage + wave * 16 * EP;            // wave-private: no further barrier needed
            const int m_w = m_base + wr * 16 * RT, n_w = nt * BN + wc * 64;
            if constexpr (LOSS) {
                static_assert(!LOSS || RT == 2 || RT == 4, "even number of row tiles: two named target sets");
                // partial sums per group of SWV2_LOSS_GROUP_ROWS = 32 rows: one group (64-row workgroups) or two (128) per wave
#pragma unroll
                for (int grp = 0; grp < RT / 2; ++grp) {
                    const int m_g = m_w + 32 * grp;
                    const int tps = (ep.d.p1 >> 2) * (ep.d.p2 >> 2);                                       // tokens per sample
                    const int b0 = fdiv(min(m_g, M - 1), tps, ep.d.mg0);                                   // sample of the group's first row
                    const bool edge = (m_g + 32 >= M) || fdiv(m_g + 32, tps, ep.d.mg0) != b0;              // the row behind the group: another sample
                    float ls[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ls2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii) {
                        const int i = 2 * grp + ii;
                        // request this row tile's targets of the NEXT N tile before this tile's stores (channels clamped inside:
                        // unconditional also behind the last N tile)
                        ep.load_tar(lrow[i], n_w + BN, ltn[i]);
                        ep.template tile_loss_t<EK == E_UNPATCH_LOSS_SKIP>(acc[i], (uint16_t*)st, lrow[i], m_w + 16 * i, n_w, lane, ls, ls2, b0, lt[i]);
                    }
                    ep.template flush<32>(ls, ls2, edge, m_g, n_w, lane);
                }
#pragma unroll
                for (int i = 0; i < RT; ++i) lt[i] = ltn[i];
                if (s + 1 < steps) commit(s + 1);
            } else {
#pragma unroll
                for (int i = 0; i < RT; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[(4 * g + r) * EP + 16 * j + fr] = acc[i][j][r];
                    ep.tile(st, m_w + i * 16, n_w, lane);
                }
            }
        } else if constexpr (LOSS) {
            if (s + 1 < steps) commit(s + 1);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Which kernel serves a product: linear_kernel_for is the ONE place that knows.  launch_nt2 switches on it, swv2_linear_kernel reports it.
// ------------------------------------------------------------------------------------------------
enum class LinearKernel {
    RESIDENT_QKV128 = SWV2_LINEAR_RESIDENT_QKV128, RESIDENT_QKV192X3 = SWV2_LINEAR_RESIDENT_QKV192X3, RESIDENT_DX128 = SWV2_LINEAR_RESIDENT_DX128,
    WIDE_DMA = SWV2_LINEAR_WIDE_DMA, WIDE = SWV2_LINEAR_WIDE, TILE64 = SWV2_LINEAR_TILE64, TILE128 = SWV2_LINEAR_TILE128
};

// Pure function of the descriptors' shape fields (no data pointer is dereferenced; rowidx / aux only as "present or not"), the internal
// kinds ak (A_*) / ek (E_*) and the value of SWV2_GEMM_WIDE.
LinearKernel linear_kernel_for(int ak, int ek, const swv2_operand* a, const swv2_epilogue* e, int N, int wide) {
    const int M = a->rows, K = a->cols;
    // the two per-block products at the benchmark width: resident-weight persistent kernel
    if (qkv_pair(ak, ek) && M >= 256 * 128 && a->rowidx) {
        if (N == 384 && K == 128 && e->p[3] == 16) return LinearKernel::RESIDENT_QKV128;
        // BASELINE configs[4] (192 channels, 8 heads in 32-wide slots): the 768 x 192 weight does not fit LDS beside an A tile, one
        // of its q / k / v parts (256 x 192 = 96 KB) does: three launches, each over all rows (the gathered fp32 rows are read three
        // times, 3 x 108 MB, against the generic kernel's re-read of the weight per 64-row tile: 207 -> 3 x ~45 us)
        if (N == 768 && K == 192 && e->p[3] == 32 && e->p[0] == 8) return LinearKernel::RESIDENT_QKV192X3;
    }
    // (its operand is fetched by LDS-DMA with 32-bit byte offsets: a larger one falls through to the tile kernels)
    if (dx_pair(ak, ek) && N == 128 && K == 384 && M >= 256 * 64 && e->rowidx && e->aux && !a->rowidx && (double)M * K * 2 < 4.29e9)
        return LinearKernel::RESIDENT_DX128;
    // wide products (K, N >= 512, N a multiple of 256): 256 x 256 tiles
    if (wide_pair(ak, ek)) {
        // BASELINE configs[4]'s d(qkv) -> dx product (N = 192, K = 768, head-major operand): one partial column tile of the DMA kernel --
        // the operand is read exactly once, the weight's 192 rows stream from L2; a quarter of the MFMAs multiply clamped rows
        // (the 64-row tile kernel re-reads the weight per tile behind a barrier per 64 k: 165 us)
        const bool part192 = dx_pair(ak, ek) && N == 192 && K == 768 && !a->rowidx && M >= 64 * WBM &&
                             (double)a->rows * a->cols * 2 < 4.29e9;                  // (only the DMA kernel clamps the weight rows)
        if (wide && (N % WBN == 0 || part192) && K % BK == 0 && (N >= 512 || part192) && K >= 512 && M >= 16 * WBM) {
            // 32-bit byte offsets in the DMA addressing: the operand below 4 GB (the weight: checked by the launcher)
            const bool small = (double)a->rows * (ak == A_HEADS ? a->cols : a->ld) * 2 < 4.29e9;
            return dma_loader(ak) && small && K % 128 == 0 && (ak == A_HEADS || !a->rowidx) ? LinearKernel::WIDE_DMA : LinearKernel::WIDE;
        }
    }
    // 64-row workgroups (one 32-row partial-sum group per wave) for the loss epilogues.  128-row workgroups (two groups per wave)
    // measured equal -- 422.8 vs 420.9 us -- with 23 registers spilled: not instantiated
    if (loss_epi(ek)) return LinearKernel::TILE64;
    // 64-row workgroups where they fill the 768 slots (3 per CU) better; only for the two per-block products
    if (qkv_pair(ak, ek) || dx_pair(ak, ek)) {
        const double w1 = cdiv(M, BM), w2 = cdiv(M, BM / 2), slots = 768.0;
        const double e1 = w1 / (std::ceil(w1 / slots) * slots), e2 = w2 / (std::ceil(w2 / slots) * slots);
        if (e2 > e1 + 0.08) return LinearKernel::TILE64;
    }
    return LinearKernel::TILE128;
}

// the internal epilogue kind (E_*) of a public one for loader kind ak, or a negative error: the pairs launch_nt1 instantiates
int linear_epi_kind(int ak, const swv2_epilogue* e) {
    static_assert(E_BF16 == SWV2_EPI_BF16 && E_BF16_GELU == SWV2_EPI_BF16_GELU && A_F32 == SWV2_OP_F32 && A_BF16_CS == SWV2_OP_BF16_CSCALE,
                  "A_* / E_* mirror the public kinds");
    if (ak == A_BF16_CS) {                         // the loss-gradient operand feeds exactly one product: d(e) = G W_head, fp32 out
        if (e->kind == SWV2_EPI_F32) return E_F32;
        swv2_set_error("swv2_linear: SWV2_OP_BF16_CSCALE supports SWV2_EPI_F32 only (got %d)", e->kind);
        return SWV2_ERR_INVALID;
    }
    if (ak == A_F32 && e->kind == SWV2_EPI_UNPATCH_LOSS) return e->p[3] ? E_UNPATCH_LOSS_SKIP : E_UNPATCH_LOSS;
    if (e->kind >= SWV2_EPI_BF16 && e->kind <= SWV2_EPI_BF16_GELU) return e->kind;        // (E_* = SWV2_EPI_* up to the loss epilogue)
    swv2_set_error("swv2_linear: unknown epilogue kind %d (or not available for operand kind %d)", e->kind, ak);
    return SWV2_ERR_INVALID;
}

// one launch shape per LinearKernel; `if constexpr` keeps each kernel to the pairs it is instantiated for (the selector returns it for no other)
template <int AK, int EK>
int launch_nt2(const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, int N, int K, hipStream_t st) {
    const LinearKernel kern = linear_kernel_for(AK, EK, a, e, N, swv2_gemm_wide());
    int rc = SWV2_OK;
    switch (kern) {
        case LinearKernel::RESIDENT_QKV128:
        case LinearKernel::RESIDENT_QKV192X3:
            if constexpr (qkv_pair(AK, EK)) rc = swv2_rw_qkv_launch(kern == LinearKernel::RESIDENT_QKV128 ? 1 : 3, a, w, e, M, st);
            break;
        case LinearKernel::RESIDENT_DX128:
            if constexpr (dx_pair(AK, EK)) rc = swv2_rw_dx128_launch(a, w, e, M, st);
            break;
        case LinearKernel::WIDE_DMA:
        case LinearKernel::WIDE:
            if constexpr (wide_pair(AK, EK)) rc = swv2_nt_wide_launch(AK, EK, kern == LinearKernel::WIDE_DMA, a, w, e, M, N, K, st);
            break;
        case LinearKernel::TILE64:
            if constexpr (qkv_pair(AK, EK) || dx_pair(AK, EK) || loss_epi(EK))
                hipLaunchKernelGGL((gemm_nt_kernel<AK, EK, BM / 2>), dim3(cdiv(M, BM / 2)), dim3(NTHREADS), 0, st, make_loader<AK>(a),
                                   (const uint16_t*)w, make_epi<EK>(e, M, N), M, N, K);
            break;
        case LinearKernel::TILE128:
            if constexpr (!loss_epi(EK))
                hipLaunchKernelGGL((gemm_nt_kernel<AK, EK>), dim3(cdiv(M, BM)), dim3(NTHREADS), 0, st, make_loader<AK>(a),
                                   (const uint16_t*)w, make_epi<EK>(e, M, N), M, N, K);
            break;
    }
    if (rc) return rc;
    SWV2_CHECK_LAUNCH("swv2_linear");
    return SWV2_OK;
}

template <int AK>
int launch_nt1(const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, int N, int K, hipStream_t st) {
    const int ek = linear_epi_kind(AK, e);
    if (ek < 0) return ek;
    // only the pairs linear_epi_kind lets through are instantiated (compile time)
    if constexpr (AK == A_BF16_CS) {
        return launch_nt2<AK, E_F32>(a, w, e, M, N, K, st);
    } else {
    if constexpr (AK == A_F32) {
        if (ek == E_UNPATCH_LOSS_SKIP) return launch_nt2<AK, E_UNPATCH_LOSS_SKIP>(a, w, e, M, N, K, st);
        if (ek == E_UNPATCH_LOSS) return launch_nt2<AK, E_UNPATCH_LOSS>(a, w, e, M, N, K, st);
    }
    switch (ek) {
        case E_BF16: return launch_nt2<AK, E_BF16>(a, w, e, M, N, K, st);
        case E_F32: return launch_nt2<AK, E_F32>(a, w, e, M, N, K, st);
        case E_F32_ACC: return launch_nt2<AK, E_F32_ACC>(a, w, e, M, N, K, st);
        case E_QKV_HEADS: return launch_nt2<AK, E_QKV_HEADS>(a, w, e, M, N, K, st);
        case E_HEADS: return launch_nt2<AK, E_HEADS>(a, w, e, M, N, K, st);
        case E_GELU_GRAD: return launch_nt2<AK, E_GELU_GRAD>(a, w, e, M, N, K, st);
        case E_UNPATCH: return launch_nt2<AK, E_UNPATCH>(a, w, e, M, N, K, st);
        case E_BF16_GELU: return launch_nt2<AK, E_BF16_GELU>(a, w, e, M, N, K, st);
    }
    return SWV2_ERR_INVALID;
    }
}

}  // namespace
extern "C" int swv2_linear_kernel(const swv2_operand* a, const swv2_epilogue* e, int N) {
    SWV2_CHECK_ARG(a && e && N > 0 && a->rows > 0 && a->cols > 0, "swv2_linear_kernel: null operand / epilogue or empty product");
    SWV2_CHECK_ARG(a->kind >= SWV2_OP_F32 && a->kind <= SWV2_OP_BF16_CSCALE, "swv2_linear_kernel: unknown operand kind %d", a->kind);
    const int ek = linear_epi_kind(a->kind, e);
    return ek < 0 ? ek : (int)linear_kernel_for(a->kind, ek, a, e, N, swv2_gemm_wide());
}

extern "C" int swv2_linear(const swv2_operand* a, const void* w_bf16, const swv2_epilogue* e, int N, void* stream) {
    int rc = check_operand(a, "swv2_linear");
    if (rc) return rc;
    SWV2_CHECK_ARG(w_bf16 && e && e->out && N > 0, "swv2_linear: null weight / epilogue / N");
    SWV2_CHECK_ARG(((uintptr_t)w_bf16 & 15) == 0 && ((uintptr_t)e->out & 15) == 0, "swv2_linear: unaligned pointer");
    if (e->kind == SWV2_EPI_BF16_GELU) SWV2_CHECK_ARG(e->aux_out != nullptr, "swv2_linear: GELU epilogue needs aux_out");
    if (e->kind == SWV2_EPI_BF16 || e->kind == SWV2_EPI_GELU_GRAD || e->kind == SWV2_EPI_BF16_GELU)
        SWV2_CHECK_ARG(e->ld % 8 == 0 && e->ld >= N, "swv2_linear: output pitch %ld must be a multiple of 8 and >= N", e->ld);
    if (e->kind == SWV2_EPI_F32 || e->kind == SWV2_EPI_F32_ACC)
        SWV2_CHECK_ARG(e->ld % 4 == 0 && e->ld >= N, "swv2_linear: output pitch %ld must be a multiple of 4 and >= N", e->ld);
    if (e->kind == SWV2_EPI_QKV_HEADS || e->kind == SWV2_EPI_HEADS)
        SWV2_CHECK_ARG(head_pad_ok(e->p[3]) && N % e->p[3] == 0 && e->p[0] > 0 && e->p[2] > 0,
                       "swv2_linear: head-split epilogue needs DP in {16,32,64,96,128,256} and N a multiple of DP (DP=%d N=%d)", e->p[3], N);
    if (e->kind == SWV2_EPI_UNPATCH || e->kind == SWV2_EPI_UNPATCH_LOSS)
        SWV2_CHECK_ARG(N == e->p[0] * 16, "swv2_linear: un-patchify needs N == Cout*16");
    if (e->kind == SWV2_EPI_UNPATCH_LOSS) {
        SWV2_CHECK_ARG(a->kind == SWV2_OP_F32, "swv2_linear: the loss epilogue takes an fp32 operand");
        SWV2_CHECK_ARG((e->p[4] == 0 || (e->p[4] >= e->p[0] && e->q[2] > 0)) && (!e->aux_out || e->ld >= e->p[0]) && e->q[2] >= 0,
                       "swv2_linear: loss epilogue: p[4] (channels of the destination tensor) needs q[2] (its dump offset), aux_out needs ld >= Cout");
        SWV2_CHECK_ARG(e->loss_tar && e->loss_qw && e->loss_part && e->loss_resid && e->q[0] >= e->q[1] + e->p[0] && e->q[1] >= 0,
                       "swv2_linear: the loss epilogue needs target, quadrature weights, sums, residual and q[1] + Cout <= q[0]");
        SWV2_CHECK_ARG((((uintptr_t)e->loss_tar | (uintptr_t)e->loss_resid) & 15) == 0, "swv2_linear: unaligned loss pointer");
        const double plane_ = (double)e->p[1] * e->p[2], nb_ = (double)a->rows / ((e->p[1] / 4) * (e->p[2] / 4));
        SWV2_CHECK_ARG((e->p[1] / 4) * (e->p[2] / 4) >= SWV2_LOSS_GROUP_ROWS, "swv2_linear: the loss epilogue needs at least %d patches per sample", SWV2_LOSS_GROUP_ROWS);
        const double cmax_ = fmax(fmax((double)e->p[3], (double)e->p[0]), fmax((double)e->p[4], e->aux_out ? (double)e->ld : 0.0));
        SWV2_CHECK_ARG(nb_ * e->q[0] * plane_ < 4.29e9 && nb_ * cmax_ * plane_ + 1024 < 4.29e9 && (double)a->rows * SWV2_LOSS_RESID_PITCH(N) + 2048 < 4.29e9 && (double)e->q[2] < 4.29e9,
                       "swv2_linear: the loss epilogue indexes its tensors with 32-bit element offsets (tensor too large)");
    }
    const int M = a->rows, K = a->cols;
    hipStream_t st = (hipStream_t)stream;
    switch (a->kind) {
        case SWV2_OP_F32: return launch_nt1<A_F32>(a, w_bf16, e, M, N, K, st);
        case SWV2_OP_BF16: return launch_nt1<A_BF16>(a, w_bf16, e, M, N, K, st);
        case SWV2_OP_BF16_GELU: return launch_nt1<A_BF16_GELU>(a, w_bf16, e, M, N, K, st);
        case SWV2_OP_HEADS: return launch_nt1<A_HEADS>(a, w_bf16, e, M, N, K, st);
        case SWV2_OP_PATCH: return launch_nt1<A_PATCH>(a, w_bf16, e, M, N, K, st);
        case SWV2_OP_MERGE_LN: return launch_nt1<A_MERGE_LN>(a, w_bf16, e, M, N, K, st);
        case SWV2_OP_BF16_CSCALE: return launch_nt1<A_BF16_CS>(a, w_bf16, e, M, N, K, st);
    }
    swv2_set_error("swv2_linear: unknown operand kind %d", a->kind);
    return SWV2_ERR_INVALID;
}

