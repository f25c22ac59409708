// Weight-gradient products of the GEMM engine: dW[N][K] += sum_m dY[m][N]^T X[m][K] (+ bias gradient).  See gemm.hip for
// the engine overview and gemm_common.h for the operand loaders shared with the NT kernels.  This file: the 128 x 128 tile body, its
// single-product and grouped kernels and their reduction; the two selectors (wgrad_kernel_for, block_wgrad_plan) and every C entry
// point of the weight gradients.  The other two kernel families sit behind plain functions declared in gemm_common.h:
// gemm_tn_wide.hip (256 x 256 tiles, one product) and gemm_tn_slab.hip (a block's four products, every operand byte fetched once).
#include "gemm_common.h"
// In-kernel phase timing (diagnostic builds only, -DSWV2_TN_STAMPS, tools/probe_tn_stamps.py): wave 0 of every workgroup
// accumulates s_memtime deltas per phase and overwrites the head of its partial tile with them (results are garbage then).
#ifdef SWV2_TN_STAMPS
#define SWV2_STAMPS
#endif
#include "stamps.h"

namespace {

// ------------------------------------------------------------------------------------------------
// TN kernel: dW[N][K] (+)= sum over a slice of rows of dY^T X ; optional db[N] = column sums of dY
// grid = (ntiles_n * ntiles_k, splits).  Output accumulated with fp32 atomics (caller zeroes dW / db).
// ------------------------------------------------------------------------------------------------
constexpr int TM = 128;                     // rows per step (4 MFMA k-steps of 32): ~100 KB in flight per workgroup
constexpr int TP = 136;                     // LDS row pitch (elements) of the [TM][128] tiles: 272 B
constexpr int TCH = TM * 16 / NTHREADS;     // 16-byte chunks per thread per operand per step (8)

struct TnOut {                 // one product's destination
    float* dW; float* db; const int32_t* nmap; const int32_t* kmap; int ldw, M, N, K, ntk, tiles; float* ws;
};
constexpr int TN_SMEM = 2 * TM * TP;        // [Y | X][TM][TP] bf16, single buffer

// one 128 x 128 output tile over the row chunks of one slice (body shared by the single-product and the grouped kernel)
// XG: the X rows are gathered through xl.d.rowidx (compile time, so the un-gathered products carry no index load at all)
template <int YK, int XK, bool XG = false, bool HINC = false>
__device__ __forceinline__ void tn_tile(const ALoad<YK>& yl, const ALoad<XK>& xl_arg, const TnOut& o, int tile, int slice,
                                        int chunk_stride, uint16_t* smem, float* dbs, uint16_t* gtab) {
    float* __restrict__ dW = o.dW;
    float* __restrict__ db = o.db;
    const int32_t* __restrict__ nmap = o.nmap;
    const int32_t* __restrict__ kmap = o.kmap;
    const int ldw = o.ldw, M = o.M, N = o.N, K = o.K, ntk = o.ntk, tiles = o.tiles;
    float* __restrict__ ws = o.ws;
    ALoad<XK> xl = xl_arg;
    if constexpr (XK == A_BF16_GELU) {          // GELU-on-load of the stored bf16 pre-activation through a lookup table
        for (int i = threadIdx.x; i < GT_N; i += NTHREADS) gtab[i] = f2bf(gelu_f(bf2f(gelu_tab_arg(i))));
        xl.tab = gtab;
        __syncthreads();
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int tn = tile / ntk, tk = tile - tn * ntk;
    const int n_base = tn * BN, k_base = tk * BN;
    // rows: slice s owns the TM-row chunks s, s + S, s + 2S, ... (S = chunk_stride = number of slices).  At any moment the S
    // slices then stream ONE contiguous S x TM-row region of dY / X, spread over every HBM channel; contiguous row ranges
    // per slice (the first version) put all slices a multiple of 256 KB .. 1 MB apart, i.e. on the same channels at the
    // same time, and the kernels sat at 2.6 - 3.0 TB/s.
    const int nchunks = (M + TM - 1) / TM;
    const int steps = (slice < chunk_stride && slice < nchunks) ? (nchunks - slice + chunk_stride - 1) / chunk_stride : 0;
    const int m_hi = M;
    const bool want_db = (db != nullptr) && (tk == 0);
    if (steps <= 0) return;
    if (tid < BN) dbs[tid] = 0.f;

    // staging: each tile is TM x 16 chunks; a thread keeps a fixed chunk column and walks rows srow + 16 i.  Operands whose
    // adjacent ROWS are adjacent in memory (the 4 x 4 patch im2col: a row is 16 bytes of each of 16 x Cin image rows) use
    // the row-fastest map instead -- thread = (row tid & 127, chunk columns (tid >> 7) + 2 i) -- so a wave reads 64
    // consecutive 16-byte groups instead of 4 rows x 16 scattered ones (PatchEmbed / head gradients: 2.9 TB/s before).
    const int srow = tid >> 4, scol = tid & 15;
    constexpr bool YRF = ALoad<YK>::ROW_FASTEST, XRF = ALoad<XK>::ROW_FASTEST;
    auto yr_ = [&](int i) { return YRF ? (tid & (TM - 1)) : srow + 16 * i; };
    auto yc_ = [&](int i) { return YRF ? (tid >> 7) + 2 * i : scol; };
    auto xr_ = [&](int i) { return XRF ? (tid & (TM - 1)) : srow + 16 * i; };
    auto xc_ = [&](int i) { return XRF ? (tid >> 7) + 2 * i : scol; };
    static_assert(TM == 128 && NTHREADS == 256, "row-fastest map: 128 rows x 2 chunk columns per pass");
    typename ALoad<YK>::Raw ry[TCH];
    typename ALoad<XK>::Raw rx[TCH];
    float colsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // Staging pipeline.  EVERY global load here is unconditional (clamped address) and the validity of a chunk travels in a
    // bit mask: rows past M and the padded rows of a window (table entry -1) are loaded from row 0 and zeroed when the
    // tile is written to LDS.  With loads under `if (row < 0) ...` -- the first version -- the compiler guarded their
    // destination registers with s_waitcnt vmcnt(0): one in the middle of issue() and one right behind the index loads of
    // resolve(), i.e. BEFORE the MFMAs, so the "prefetch" of the next step was waited for at once and the kernel ran
    // load -> wait -> compute in series (2.6 - 3.2 TB/s; found in the ISA, tools/probe_tn_stamps.py showed 40 % in issue).
    // Gathered X rows: the table entries of step s + 2 are fetched behind the data loads of step s + 1 and consumed one
    // iteration later, by which time they have long arrived.
    int yrow[TCH], xrow[TCH];          // source rows of the next issue (X gathered: raw table entries)
    uint32_t xin = 0;                  // X gathered: bit i = chunk row i of the next issue lies inside [0, M)
    uint32_t okmask = 0;               // chunks in flight: bit i = Y chunk i valid, bit 16 + i = X chunk i valid
    // LINEAR operands (plain row-major rows, not gathered): chunk i of a step sits at  (m0 + srow + 16 i) * ld + column  -- one
    // 32-bit multiply per operand and step, then adds.  Formed per chunk as  ptr + (long)row * ld + k  the staging loop carried
    // 64 v_mul_lo_u32 + 40 v_mad_u64_u32 + 8 v_mul_hi per step (quarter-rate instructions: about as many vector-issue cycles as the
    // step's 64 MFMAs, found in the ISA of the grouped kernel); chunks past M load from the operand's first rows (masked at commit).
    constexpr bool YLIN = ALoad<YK>::LINEAR && !YRF, XLIN = ALoad<XK>::LINEAR && !XRF && !XG;
    const uint32_t ycol = (uint32_t)min(n_base + scol * 8, max(N - 8, 0)), xcol = (uint32_t)min(k_base + scol * 8, max(K - 8, 0));
    const uint32_t ystep = 16u * (uint32_t)yl.d.ld, xstep = 16u * (uint32_t)xl.d.ld;
    uint32_t yoff0 = 0, xoff0 = 0;     // element offset of chunk 0 of the next issue
    // head-major operands ([Bw][h][S][Lp][DP]): the window / token split once per step, then adds (ALoad<A_HEADS>::Step); needs a
    // step (TM rows) to span at most one window boundary
    // (HINC: selected by the kernel when Lp >= TM; column offsets of masked chunks: the operand's first row)
    constexpr bool YHD = YK == A_HEADS && HINC, XHD = XK == A_HEADS && HINC;
    typename ALoad<A_HEADS>::Step yst = {0u, 0}, xst = {0u, 0};
    auto resolve = [&](int s) {
        xin = 0;
        if constexpr (YLIN || XLIN || YHD || XHD) {
            const int m0 = (slice + s * chunk_stride) * TM + srow;
            if constexpr (YLIN) yoff0 = (uint32_t)m0 * (uint32_t)yl.d.ld + ycol;
            if constexpr (XLIN) xoff0 = (uint32_t)m0 * (uint32_t)xl.d.ld + xcol;
            if constexpr (YHD) yst = yl.step_base(min(m0, M - 1), (int)ycol);
            if constexpr (XHD) xst = xl.step_base(min(m0, M - 1), (int)xcol);
        }
#pragma unroll
        for (int i = 0; i < TCH; ++i) {
            const int m0 = (slice + s * chunk_stride) * TM, my = m0 + yr_(i), mx = m0 + xr_(i);
            const bool iny = (s < steps) && (my < m_hi), inx = (s < steps) && (mx < m_hi);
            yrow[i] = iny ? my : -1;
            if constexpr (XG) {
                xrow[i] = xl.d.rowidx[min(mx, M - 1)];
                xin |= (uint32_t)inx << i;
            } else {
                xrow[i] = inx ? mx : -1;
            }
        }
    };
    auto issue = [&](int s) {
        okmask = 0;
#pragma unroll
        for (int i = 0; i < TCH; ++i) {
            const int yk = n_base + yc_(i) * 8, xk = k_base + xc_(i) * 8;
            const int xr = XG ? (((xin >> i) & 1) ? xrow[i] : -1) : xrow[i];
            const bool yok = yrow[i] >= 0 && yk < N, xok = xr >= 0 && xk < K;
            if constexpr (YLIN) ry[i] = yl.raw_lin(yrow[i] >= 0 ? yoff0 + i * ystep : ycol);
            else if constexpr (YHD) ry[i] = yl.raw_lin(yrow[i] >= 0 ? yl.step_off(yst, i) : 0u);
            else ry[i] = yl.raw_unc(max(yrow[i], 0), yk < N ? yk : 0);
            if constexpr (XLIN) rx[i] = xl.raw_lin(xr >= 0 ? xoff0 + i * xstep : xcol);
            else if constexpr (XHD) rx[i] = xl.raw_lin(xr >= 0 ? xl.step_off(xst, i) : 0u);
            else if constexpr (XG && XK == A_F32) rx[i] = xl.raw_lin((uint32_t)max(xr, 0) * (uint32_t)xl.d.ld + xcol);     // gathered rows: one 32-bit multiply
            else rx[i] = xl.raw_unc(max(xr, 0), xk < K ? xk : 0);
            okmask |= ((uint32_t)yok << i) | ((uint32_t)xok << (16 + i));
        }
    };
    auto commit = [&]() {
        uint16_t* Ys = smem;
        uint16_t* Xs = smem + TM * TP;
        const uint4 zero4 = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TCH; ++i) {
            const uint4 yv = ((okmask >> i) & 1) ? yl.cvt(ry[i]) : zero4;
            *(uint4*)(Ys + yr_(i) * TP + yc_(i) * 8) = yv;
            *(uint4*)(Xs + xr_(i) * TP + xc_(i) * 8) = ((okmask >> (16 + i)) & 1) ? xl.cvt(rx[i]) : zero4;
            if (want_db && !YRF) {                       // (a row-fastest dY has no fixed column per thread: rejected by the launcher)
                float v[8];
                unpack8(yv, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) colsum[e] += v[e];
            }
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    STAMP_DECL(8)
    STAMP_START();
    resolve(0);
    issue(0);
    resolve(1);
    STAMP(7);
    for (int s = 0; s < steps; ++s) {
        STAMP_WAITV();
        STAMP(0);
        commit();
        STAMP(1);
        __syncthreads();
        STAMP(2);
        if (s + 1 < steps) { issue(s + 1); resolve(s + 2); }
        STAMP(3);
        const uint16_t* Ys = smem;
        const uint16_t* Xs = smem + TM * TP;
        // A operand = dY^T (rows n, k = m), B operand = X (k = m, cols k'): both are transposed reads of row-major tiles
        // (the K = 32 fragment, two transposed reads joined, is open-coded in all three families: see gemm_tn_wide_kernel)
#pragma unroll
        for (int kk = 0; kk < TM / 32; ++kk) {
            bf16x8 af[4], bf[4];
            const int r0 = 32 * kk + 8 * g + (fr >> 2), cc = (fr & 3) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x4 a0 = lds_tr_read(Ys + r0 * TP + wr * 64 + i * 16 + cc);
                const bf16x4 a1 = lds_tr_read(Ys + (r0 + 4) * TP + wr * 64 + i * 16 + cc);
                const bf16x4 b0 = lds_tr_read(Xs + r0 * TP + wc * 64 + i * 16 + cc);
                const bf16x4 b1 = lds_tr_read(Xs + (r0 + 4) * TP + wc * 64 + i * 16 + cc);
                af[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                bf[i] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma32(af[i], bf[j], acc[i][j]);
        }
        asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[3][3][3]));
        STAMP(4);
        __syncthreads();                    // all waves done with the tile before the next commit overwrites it
        STAMP(5);
    }
    // accumulate the tile: rows n = n_base + wr*64 + 16i + 4g + r, cols k = k_base + wc*64 + 16j + fr
    if (ws) {                               // workspace path: plain partial tile, summed by tn_reduce_kernel
        float* pt = ws + ((size_t)slice * tiles + tile) * (BN * BN);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pt[(wr * 64 + 16 * i + 4 * g + r) * BN + wc * 64 + 16 * j + fr] = acc[i][j][r];
#ifdef SWV2_TN_STAMPS
        STAMP_WAITV();
        STAMP(6);
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) ((unsigned long long*)pt)[k] = st_acc[k];
        }
#endif
    } else
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int n = n_base + wr * 64 + 16 * i + 4 * g + r, k = k_base + wc * 64 + 16 * j + fr;
                if (n >= N || k >= K) continue;
                n = wg_index(nmap, n);
                k = wg_index(kmap, k);
                if (n >= 0 && k >= 0) atomicAdd(dW + (long)n * ldw + k, acc[i][j][r]);
            }
    if (want_db) {
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(&dbs[scol * 8 + e], colsum[e]);
        __syncthreads();
        if (tid < BN && n_base + tid < N) {
            const int n = wg_index(nmap, n_base + tid);
            if (n >= 0) atomicAdd(db + n, dbs[tid]);
        }
    }
}

// single product: grid = tiles * slices (slices padded to a multiple of 8)
// XCD-aware block -> (tile, row slice) map.  Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one), and
// the tiles of one row slice re-read the same dY / X rows: give all tiles of a slice consecutive slots on ONE XCD so
// the re-reads hit that XCD's L2 instead of HBM (PMC before: 415 MB vs 198 MB algorithmic for the fc1 gradient).
// Speed only, never correctness.
template <int YK, int XK, bool XG>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_kernel(ALoad<YK> yl, ALoad<XK> xl, TnOut o, int chunk_stride) {
    __shared__ __attribute__((aligned(16))) uint16_t smem[TN_SMEM];
    __shared__ float dbs[BN];
    __shared__ __attribute__((aligned(16))) uint16_t gtab[XK == A_BF16_GELU ? GT_N : 8];
    const int lin = blockIdx.x;                       // 1-D launch: lin = xcd + 8 * (q * tiles + tile)
    const int x8 = lin & 7, rest = lin >> 3;
    const int tile = rest % o.tiles, slice = (rest / o.tiles) * 8 + x8;
    tn_tile<YK, XK, XG>(yl, xl, o, tile, slice, chunk_stride, smem, dbs, gtab);
}

// The four weight-gradient products of one transformer block in ONE launch (fc2, fc1, proj, qkv: 4 + 4 + 1 + 3 tiles at
// C = 128).  Measured on the separate launches (bench.py at local batch 1 / 2 / 4, tools/batch_fit.py): each costs
// ~13 - 16 us independent of the row count (ramp, first-load latency, partial-tile drain) on top of ~4.3 us per 128-row
// step, i.e. 2.6 - 3.2 TB/s at 8 steps per workgroup but 5.8 TB/s marginal.  Grouped, every workgroup walks ~25 steps and
// the fixed part is paid once; one tn_group_reduce launch replaces four tn_reduce launches.
struct TnGroup {
    ALoad<A_BF16> y0; ALoad<A_BF16_GELU> x0;      // fc2:  d(a2)^T GELU(hpre)
    ALoad<A_BF16> y1; ALoad<A_F32> x1;            // fc1:  d(h)^T x1
    ALoad<A_BF16> y2; ALoad<A_HEADS> x2;          // proj: d(a1)^T merge(oh)
    ALoad<A_HEADS> y3; ALoad<A_F32> x3;           // qkv:  d(qkv)^T gather(x)
    TnOut o[4];
    int first[5];                                 // first global tile index of each product; first[4] = total
    int slices;
};
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_group_kernel(TnGroup a) {
    __shared__ __attribute__((aligned(16))) uint16_t smem[TN_SMEM];
    __shared__ float dbs[BN];
    __shared__ __attribute__((aligned(16))) uint16_t gtab[GT_N];
    const int lin = blockIdx.x, x8 = lin & 7, rest = lin >> 3, tt = a.first[4];
    const int t = rest % tt, slice = (rest / tt) * 8 + x8;
    if (t < a.first[1]) tn_tile<A_BF16, A_BF16_GELU>(a.y0, a.x0, a.o[0], t, slice, a.slices, smem, dbs, gtab);
    else if (t < a.first[2]) tn_tile<A_BF16, A_F32>(a.y1, a.x1, a.o[1], t - a.first[1], slice, a.slices, smem, dbs, gtab);
    else if (a.x2.d.p2 >= TM) {       // head-major operands walked incrementally (a step spans at most one window boundary)
        if (t < a.first[3]) tn_tile<A_BF16, A_HEADS, false, true>(a.y2, a.x2, a.o[2], t - a.first[2], slice, a.slices, smem, dbs, gtab);
        else tn_tile<A_HEADS, A_F32, true, true>(a.y3, a.x3, a.o[3], t - a.first[3], slice, a.slices, smem, dbs, gtab);
    } else {
        if (t < a.first[3]) tn_tile<A_BF16, A_HEADS>(a.y2, a.x2, a.o[2], t - a.first[2], slice, a.slices, smem, dbs, gtab);
        else tn_tile<A_HEADS, A_F32, true>(a.y3, a.x3, a.o[3], t - a.first[3], slice, a.slices, smem, dbs, gtab);
    }
}

// ------------------------------------------------------------------------------------------------
// Second stage of the workspace path: dW[nmap(n)][kmap(k)] += sum over row slices of the partial tiles
// ws[slice][tile][128][128].  Device-scope float atomics resolve beyond the per-XCD L2s and cost ~5 ns each when 64+
// workgroups hit the same 64 K addresses (measured: the fc1 gradient went 94 -> 177 us from 64 to 256 slices), so with
// a workspace the slices write plain coalesced partials and this kernel owns every output element exclusively.
// block = 256 threads = 64 tile entries x 4 slice groups.
// ------------------------------------------------------------------------------------------------
struct TnReduce { TnOut o[4]; int first[5]; int slices; };
__global__ __launch_bounds__(256) void tn_reduce_kernel(TnReduce a) {
    __shared__ float part[4][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), sg = threadIdx.x >> 6, gt = blockIdx.y;
    const int pi = (gt >= a.first[1]) + (gt >= a.first[2]) + (gt >= a.first[3]);
    const TnOut& o = a.o[pi];
    const int tile = gt - a.first[pi], tiles = o.tiles, ntk = o.ntk;
    const int slices = min(a.slices, (o.M + TM - 1) / TM);
    const float* src = o.ws + (size_t)tile * (BN * BN) + e;
    const size_t stride = (size_t)tiles * (BN * BN);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int sl = sg;
    for (; sl + 12 < slices; sl += 16) {
        s0 += src[(size_t)sl * stride];
        s1 += src[(size_t)(sl + 4) * stride];
        s2 += src[(size_t)(sl + 8) * stride];
        s3 += src[(size_t)(sl + 12) * stride];
    }
    for (; sl < slices; sl += 4) s0 += src[(size_t)sl * stride];
    part[sg][threadIdx.x & 63] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sg == 0) {
        const int tn = tile / ntk, tk = tile - tn * ntk;
        int n = tn * BN + (e >> 7), k = tk * BN + (e & 127);
        if (n < o.N && k < o.K) {
            n = wg_index(o.nmap, n);
            k = wg_index(o.kmap, k);
            const int l = threadIdx.x;
            if (n >= 0 && k >= 0) o.dW[(long)n * o.ldw + k] += (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
        }
    }
}

struct TnPlan { int ntn, ntk, tiles, real_slices, slices; size_t ws_bytes; };
TnPlan tn_plan(int M, int N, int K, int splits) {
    TnPlan p;
    p.ntn = cdiv(N, BN); p.ntk = cdiv(K, BN); p.tiles = p.ntn * p.ntk;
    int eff = (p.tiles >= 3) ? splits : splits * 2;               // small outputs: more row slices to fill the chip
    // large outputs need few: 128 slices of a 768 x 3072 gradient (144 tiles) were 18 432 workgroups writing 1.2 GB of
    // partial tiles, and the reduction launch cost as much as a GEMM -- two rounds of workgroups (1024) are plenty
    eff = std::min(eff, std::max(8, (1024 / p.tiles) / 8 * 8));
    p.real_slices = std::min(eff, cdiv(M, TM));
    p.slices = cdiv(p.real_slices, 8) * 8;                        // padded to a multiple of 8 (empty slices exit at once)
    p.ws_bytes = (size_t)p.real_slices * p.tiles * BN * BN * sizeof(float);
    return p;
}
TnOut tn_out(const swv2_wgrad_item& it, float* ws) {
    TnOut o;
    o.dW = it.dW; o.db = it.db; o.nmap = it.nmap; o.kmap = it.kmap; o.ldw = it.ldw; o.M = it.dy.rows; o.N = it.dy.cols; o.K = it.x.cols;
    o.ntk = cdiv(o.K, BN); o.tiles = cdiv(o.N, BN) * o.ntk; o.ws = ws;
    return o;
}

// ------------------------------------------------------------------------------------------------
// Which kernel serves a weight gradient: wgrad_kernel_for is the ONE place that knows.  launch_tn switches on it,
// swv2_linear_wgrad_kernel reports it.
// ------------------------------------------------------------------------------------------------
enum class WgradKernel { WIDE = SWV2_WGRAD_WIDE, TILE = SWV2_WGRAD_TILE };

// Pure function of the operands' shape fields (rowidx only as "present or not"), the workspace size (0 = none: the atomic path) and the
// value of SWV2_GEMM_WIDE.  Wide widths: 256 x 256 tiles by LDS-DMA (gemm_tn_wide.hip), workspace path only; the operands raw bf16 (dY never
// gathered, not both head-major) or fp32 X rows, which are cast -- and gathered -- into the workspace first.
WgradKernel wgrad_kernel_for(const swv2_operand* y, const swv2_operand* x, size_t ws_bytes, int wide) {
    const int yk = y->kind, xk = x->kind;
    const bool kinds = (yk == A_BF16 || yk == A_HEADS) && (xk == A_BF16 || xk == A_HEADS || xk == A_F32) && !(yk == A_HEADS && xk == A_HEADS) &&
                       !y->rowidx && (xk == A_F32 || !x->rowidx);
    const size_t need = swv2_tn_wide_ws_bytes(y->rows, y->cols, x->cols);
    return wide && need && kinds && ws_bytes >= need ? WgradKernel::WIDE : WgradKernel::TILE;
}

// the 128 x 128 tile kernel: fp32 atomics on dW (ws == NULL) or per-slice partial tiles + tn_reduce_kernel
template <int YK, int XK>
int launch_tn_tile(const swv2_wgrad_item& it, int splits, float* ws, size_t ws_bytes, hipStream_t st) {
    const swv2_operand *y = &it.dy, *x = &it.x;
    const TnPlan p = tn_plan(y->rows, y->cols, x->cols, splits);
    if (ws && ws_bytes < p.ws_bytes) {
        swv2_set_error("swv2_linear_wgrad_ws: workspace of %zu bytes, %zu needed (swv2_linear_wgrad_ws_bytes)", ws_bytes, p.ws_bytes);
        return SWV2_ERR_INVALID;
    }
    const TnOut o = tn_out(it, ws);
    // gathered operands: dY never; X only as fp32 rows (the qkv gradient's window gather)
    if (y->rowidx || (x->rowidx && XK != A_F32)) {
        swv2_set_error("swv2_linear_wgrad: a row gather is supported for a fp32 X operand only (dY kind %d, X kind %d)", y->kind, x->kind);
        return SWV2_ERR_UNSUPPORTED;
    }
    if constexpr (XK == A_F32) {
        if (x->rowidx)
            hipLaunchKernelGGL((gemm_tn_kernel<YK, XK, true>), dim3(p.tiles * p.slices), dim3(NTHREADS), 0, st, make_loader<YK>(y),
                               make_loader<XK>(x), o, p.real_slices);
        else
            hipLaunchKernelGGL((gemm_tn_kernel<YK, XK, false>), dim3(p.tiles * p.slices), dim3(NTHREADS), 0, st, make_loader<YK>(y),
                               make_loader<XK>(x), o, p.real_slices);
    } else {
        hipLaunchKernelGGL((gemm_tn_kernel<YK, XK, false>), dim3(p.tiles * p.slices), dim3(NTHREADS), 0, st, make_loader<YK>(y),
                           make_loader<XK>(x), o, p.real_slices);
    }
    if (ws) {
        TnReduce r = {};
        r.o[0] = o; r.first[0] = 0; r.first[1] = r.first[2] = r.first[3] = r.first[4] = p.tiles; r.slices = p.real_slices;
        hipLaunchKernelGGL(tn_reduce_kernel, dim3(BN * BN / 64, p.tiles), dim3(256), 0, st, r);
    }
    SWV2_CHECK_LAUNCH("swv2_linear_wgrad");
    return SWV2_OK;
}

// one product whose (dY, X) pair the tile kernel is instantiated for: the kernel wgrad_kernel_for names
template <int YK, int XK>
int launch_tn(const swv2_wgrad_item& it, int splits, void* ws, size_t ws_bytes, hipStream_t st) {
    switch (wgrad_kernel_for(&it.dy, &it.x, ws ? ws_bytes : 0, swv2_gemm_wide())) {
        case WgradKernel::WIDE: return swv2_tn_wide_launch(it, ws, st);
        case WgradKernel::TILE: break;
    }
    return launch_tn_tile<YK, XK>(it, splits, (float*)ws, ws_bytes, st);
}

// only the (dY, X) operand pairs that occur in the model are instantiated (compile time): any dY kind with fp32 X rows, bf16 dY with
// the bf16 kinds and the patch layout, fp32 dY with the PatchMerging operand
int launch_wgrad(const swv2_wgrad_item& it, int splits, void* ws, size_t ws_bytes, hipStream_t st) {
#define SWV2_TN(YK_, XK_) return launch_tn<YK_, XK_>(it, splits, ws, ws_bytes, st)
    const int xk = it.x.kind;
    switch (it.dy.kind) {
        case SWV2_OP_F32:
            if (xk == SWV2_OP_F32) SWV2_TN(A_F32, A_F32);
            if (xk == SWV2_OP_MERGE_LN) SWV2_TN(A_F32, A_MERGE_LN);
            break;
        case SWV2_OP_BF16:
            switch (xk) {
                case SWV2_OP_F32: SWV2_TN(A_BF16, A_F32);
                case SWV2_OP_BF16: SWV2_TN(A_BF16, A_BF16);
                case SWV2_OP_BF16_GELU: SWV2_TN(A_BF16, A_BF16_GELU);
                case SWV2_OP_HEADS: SWV2_TN(A_BF16, A_HEADS);
                case SWV2_OP_PATCH: SWV2_TN(A_BF16, A_PATCH);
            }
            break;
        case SWV2_OP_HEADS: if (xk == SWV2_OP_F32) SWV2_TN(A_HEADS, A_F32); break;
        case SWV2_OP_PATCH: if (xk == SWV2_OP_F32) SWV2_TN(A_PATCH, A_F32); break;
        case SWV2_OP_BF16_CSCALE: if (xk == SWV2_OP_F32) SWV2_TN(A_BF16_CS, A_F32); break;
        default:
            swv2_set_error("swv2_linear_wgrad: unsupported dY operand kind %d", it.dy.kind);
            return SWV2_ERR_INVALID;
    }
#undef SWV2_TN
    swv2_set_error("swv2_linear_wgrad: operand pair (dY kind %d, X kind %d) is not instantiated", it.dy.kind, it.x.kind);
    return SWV2_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" size_t swv2_linear_wgrad_ws_bytes(int M, int N, int K, int splits) {
    if (!(M > 0 && N > 0 && K > 0 && splits > 0)) return 0;
    return std::max(tn_plan(M, N, K, splits).ws_bytes, swv2_tn_wide_ws_bytes(M, N, K));
}

// one weight gradient as the engine sees it: an item, the row slices, the workspace (common.h; swv2_block_bwd hands its items over as they are)
int swv2_wgrad_launch(const swv2_wgrad_item& it, int splits, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_operand(&it.dy, "swv2_linear_wgrad(dy)");
    if (rc) return rc;
    rc = check_operand(&it.x, "swv2_linear_wgrad(x)");
    if (rc) return rc;
    SWV2_CHECK_ARG(it.dW && splits > 0 && it.ldw > 0, "swv2_linear_wgrad: null dW, non-positive splits or bad pitch");
    SWV2_CHECK_ARG(it.dy.rows == it.x.rows, "swv2_linear_wgrad: row counts differ (%d vs %d)", it.dy.rows, it.x.rows);
    SWV2_CHECK_ARG(!(it.db && it.dy.kind == SWV2_OP_PATCH), "swv2_linear_wgrad: no bias gradient with a patch-layout dY (row-fastest staging)");
    return launch_wgrad(it, splits, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int swv2_linear_wgrad_ws(const swv2_operand* dy, const swv2_operand* x, float* dW, float* db, const int32_t* nmap,
                                    const int32_t* kmap, int ldw, int splits, void* ws, size_t ws_bytes, void* stream) {
    SWV2_CHECK_ARG(dy && x, "swv2_linear_wgrad(%s): null operand", dy ? "x" : "dy");
    const swv2_wgrad_item it = {*dy, *x, dW, db, nmap, kmap, ldw};
    return swv2_wgrad_launch(it, splits, ws, ws_bytes, stream);
}

extern "C" int swv2_linear_wgrad(const swv2_operand* dy, const swv2_operand* x, float* dW, float* db, const int32_t* nmap,
                                 const int32_t* kmap, int ldw, int splits, void* stream) {
    return swv2_linear_wgrad_ws(dy, x, dW, db, nmap, kmap, ldw, splits, nullptr, 0, stream);
}

extern "C" int swv2_linear_wgrad_kernel(const swv2_operand* dy, const swv2_operand* x, int splits, size_t ws_bytes) {
    SWV2_CHECK_ARG(dy && x && splits > 0 && dy->rows > 0 && dy->rows == x->rows, "swv2_linear_wgrad_kernel: null operand, non-positive splits or row mismatch");
    return (int)wgrad_kernel_for(dy, x, ws_bytes, swv2_gemm_wide());       // (splits shapes the tile kernel's plan, not the choice)
}

// ------------------------------------------------------------------------------------------------
// grouped launch: the four weight gradients of one block (see gemm_tn_group_kernel)
// ------------------------------------------------------------------------------------------------
namespace {
// the grouped tile kernel's plan for four products of N[i] x K[i] outputs: first global tile of each (first[4] = all tiles), the row
// slices (requested, or 0 = two workgroups -- 70 KB of LDS each -- per CU, one round; a multiple of 8) and the partial tiles' bytes
struct GroupPlan { int first[5]; int slices; size_t bytes; };
GroupPlan group_plan(const int N[4], const int K[4], int requested) {
    GroupPlan g = {};
    int tt = 0;
    for (int i = 0; i < 4; ++i) {
        g.first[i] = tt;
        tt += cdiv(N[i], BN) * cdiv(K[i], BN);
    }
    g.first[4] = tt;
    g.slices = requested > 0 ? std::max(8, requested / 8 * 8) : std::max(8, (2 * 256 / tt) / 8 * 8);
    g.bytes = (size_t)g.slices * tt * BN * BN * sizeof(float);
    return g;
}
GroupPlan group_plan(const swv2_wgrad_item* it, int requested) {
    const int N[4] = {it[0].dy.cols, it[1].dy.cols, it[2].dy.cols, it[3].dy.cols}, K[4] = {it[0].x.cols, it[1].x.cols, it[2].x.cols, it[3].x.cols};
    return group_plan(N, K, requested);
}
}  // namespace

extern "C" size_t swv2_block_wgrad_ws_bytes(int C, int hidden, int heads_dp, int slices) {
    if (C <= 0 || hidden <= 0 || heads_dp <= 0) return 0;
    const int N[4] = {C, hidden, C, 3 * heads_dp}, K[4] = {hidden, C, heads_dp, C};       // fc2, fc1, proj, qkv
    return std::max(group_plan(N, K, slices).bytes, swv2_tn_slab_ws_bytes(C, hidden, heads_dp));
}

extern "C" int swv2_block_wgrad(const swv2_wgrad_item* it, int slices, void* ws, size_t ws_bytes, void* stream) {
    return swv2_block_wgrad_ln(it, slices, ws, ws_bytes, nullptr, stream);
}

namespace {
// Which kernel runs a block's four products, and its plan: the ONE place that knows.  Second-generation kernel (gemm_tn_slab.hip:
// operands fetched once, by LDS-DMA) for the shapes, workspace and CU count it covers; an explicit slice count selects the 128 x 128
// tile kernel.  cus = 0: the current device's.
swv2_block_wgrad_plan_t block_wgrad_plan(const swv2_wgrad_item* it, int slices, size_t ws_bytes, int cus) {
    swv2_block_wgrad_plan_t p = {};
    if (slices <= 0 && swv2_tn_slab_covers(it, ws_bytes, cus, &p)) {
        p.kernel = SWV2_BLOCK_WGRAD_SLAB;
        return p;
    }
    const GroupPlan g = group_plan(it, slices);
    p = {};
    p.kernel = SWV2_BLOCK_WGRAD_GROUPED;
    for (int i = 0; i < 4; ++i) { p.S[i] = g.slices; p.SR[i] = TM; p.wgs[i] = (g.first[i + 1] - g.first[i]) * g.slices; }
    p.bytes = g.bytes;
    return p;
}

// gemm_tn_group_kernel + tn_reduce_kernel over the four items (already checked)
int launch_tn_group(const swv2_wgrad_item* it, int slices, void* ws, size_t ws_bytes, const swv2_ln_partials* ln, hipStream_t st) {
    const GroupPlan gp = group_plan(it, slices);
    const int tt = gp.first[4], S = gp.slices;
    SWV2_CHECK_ARG(ws_bytes >= gp.bytes, "swv2_block_wgrad: workspace of %zu bytes, %zu needed", ws_bytes, gp.bytes);
    // (the tile kernel's reduction carries no rider.  Launched only after every argument check: an error return must not leave the
    // LayerNorm gradients accumulated and the weight gradients not -- ADVICE r4)
    if (ln && ln->C > 0)
        swv2_launch_ln_partials_reduce2(ln->ws[0], ln->dgamma[0], ln->dbeta[0], ln->n[0], ln->ws[1], ln->dgamma[1], ln->dbeta[1], ln->n[1], ln->C, st);
    TnGroup g = {};
    TnReduce r = {};
    for (int i = 0; i < 4; ++i) r.o[i] = g.o[i] = tn_out(it[i], (float*)ws + (size_t)gp.first[i] * S * BN * BN);
    for (int i = 0; i < 5; ++i) r.first[i] = g.first[i] = gp.first[i];
    g.y0 = make_loader<A_BF16>(&it[0].dy); g.x0 = make_loader<A_BF16_GELU>(&it[0].x);
    g.y1 = make_loader<A_BF16>(&it[1].dy); g.x1 = make_loader<A_F32>(&it[1].x);
    g.y2 = make_loader<A_BF16>(&it[2].dy); g.x2 = make_loader<A_HEADS>(&it[2].x);
    g.y3 = make_loader<A_HEADS>(&it[3].dy); g.x3 = make_loader<A_F32>(&it[3].x);
    g.slices = r.slices = S;
    hipLaunchKernelGGL(gemm_tn_group_kernel, dim3(tt * S), dim3(NTHREADS), 0, st, g);
    hipLaunchKernelGGL(tn_reduce_kernel, dim3(BN * BN / 64, tt), dim3(256), 0, st, r);
    SWV2_CHECK_LAUNCH("swv2_block_wgrad");
    return SWV2_OK;
}
}  // namespace

extern "C" int swv2_block_wgrad_plan(const swv2_wgrad_item* it, int slices, size_t ws_bytes, int cus, swv2_block_wgrad_plan_t* out) {
    SWV2_CHECK_ARG(it && out && cus >= 0, "swv2_block_wgrad_plan: null items or answer, or a negative CU count");
    *out = block_wgrad_plan(it, slices, ws_bytes, cus);
    return SWV2_OK;
}

extern "C" int swv2_block_wgrad_kernel(const swv2_wgrad_item* it, int slices, size_t ws_bytes) {
    SWV2_CHECK_ARG(it, "swv2_block_wgrad_kernel: null items");
    return block_wgrad_plan(it, slices, ws_bytes, 0).kernel;
}

int swv2_block_wgrad_ln(const swv2_wgrad_item* it, int slices, void* ws, size_t ws_bytes, const swv2_ln_partials* ln, void* stream) {
    SWV2_CHECK_ARG(it && ws, "swv2_block_wgrad: null items or workspace");
    static const int want[4][2] = {{SWV2_OP_BF16, SWV2_OP_BF16_GELU}, {SWV2_OP_BF16, SWV2_OP_F32}, {SWV2_OP_BF16, SWV2_OP_HEADS},
                                   {SWV2_OP_HEADS, SWV2_OP_F32}};
    for (int i = 0; i < 4; ++i) {
        int rc = check_operand(&it[i].dy, "swv2_block_wgrad(dy)");
        if (rc) return rc;
        rc = check_operand(&it[i].x, "swv2_block_wgrad(x)");
        if (rc) return rc;
        SWV2_CHECK_ARG(it[i].dy.kind == want[i][0] && it[i].x.kind == want[i][1],
                       "swv2_block_wgrad: item %d must be (dY kind %d, X kind %d)", i, want[i][0], want[i][1]);
        SWV2_CHECK_ARG(it[i].dW && it[i].ldw > 0 && it[i].dy.rows == it[i].x.rows, "swv2_block_wgrad: item %d: null dW or row mismatch", i);
        SWV2_CHECK_ARG(!it[i].dy.rowidx && (i == 3 ? it[i].x.rowidx != nullptr : it[i].x.rowidx == nullptr),
                       "swv2_block_wgrad: item %d: only the qkv product's X rows are gathered (and they must be)", i);
    }
    switch (block_wgrad_plan(it, slices, ws_bytes, 0).kernel) {
        case SWV2_BLOCK_WGRAD_SLAB: return swv2_tn_slab_launch(it, ws, ws_bytes, ln, (hipStream_t)stream);
        case SWV2_BLOCK_WGRAD_GROUPED: break;
    }
    return launch_tn_group(it, slices, ws, ws_bytes, ln, (hipStream_t)stream);
}
