// The resident-weight row GEMMs of a block at the benchmark width (gfx950 / CDNA4): two bodies of gemm_rw_kernel that share no pipeline.
// The second one in this file serves the qkv product (weight in LDS; described at the kernel).  The first is the streaming body for a
// block's d(qkv) -> dx product at C = 128 (N = 128, K = 384):
//   dx[rowidx[m]][0..127] = (dqkv[m][0..383] . W^T + bias) + residual[rowidx[m]][0..127]
// The qkv body keeps the weight in LDS and runs its phases in series per row tile (wait for the register-
// staged rows, commit, barrier, MFMAs, barrier, epilogue, barrier).  Here nothing is staged through registers and nothing waits for
// the tile it is about to use:
//   * the weight lives in REGISTERS: wave w owns output columns 16 w .. 16 w + 15 and holds their B fragments of all 12 k-steps
//     (48 VGPRs) for the whole kernel; every wave multiplies all 32 rows of a stage against its own columns, k-steps ascending into
//     one accumulator per 16 x 16 tile, so every output element sees the accumulation chain of the tile kernels (bit-identical)
//   * rows reach LDS by LDS-DMA (global_load_lds_dwordx4) in stages of 32 rows, D = NS - 1 stages in flight:
//       A stage     [24 column blocks][32 rows][32 B] bf16 (24 KB).  For one (head, part) 32 consecutive rows of a window are 1 KB
//                   contiguous = one wave instruction; rows that straddle a window (or heads wider than 16) use the per-lane source address
//       residual    [32 rows][128] fp32 (16 KB): the rows the stage's results are added to, fetched through the scatter table; wave w
//                   fetches rows 4 w .. 4 w + 3 and later stores exactly these rows
//       index       the scatter entries of a stage, one dword per lane (the lane's own row), fetched D stages ahead of the residual
//                   rows that need them as addresses, so that the wait which retires stage t also retires the entries of stage t + D
//   * A fragments: lane (fr, g) of k-step ks reads 16 B at block (2 ks + g / 2), row fr, half g & 1.  A ds_read_b128 lane group (16
//     lanes: fr 0-3 | 12-15 with one g, fr 4-11 with the next) covers offsets 32 fr + 16 (g & 1) mod 256: 16 different 16-byte slots
//     of the 256-byte bank row, so the layout as it lands is conflict-free and needs no swizzle
//   * the epilogue has no staging area: each wave adds its 32 x 16 results (+ bias) INTO the stage's residual tile in LDS --
//     (acc + bias) + residual, the order of Epi<E_F32> -- and after one barrier every wave stores its own four rows as full 512-byte
//     rows.  16-byte piece p of row r sits at position p ^ (4 * ((r >> 2) & 1)) (permuted on the SOURCE side of the DMA): the
//     dword read-modify-writes of a half wave (two 4-row groups x 16 columns) then touch 32 different banks
//   * one hand-over per stage: a counted s_waitcnt vmcnt(N) + a raw s_barrier (never __syncthreads: it would drain the DMA queue).
//     The loop holds no ordinary global load.  The row stores enter the same in-order queue behind the stage's DMAs; a store whose
//     lanes are all masked (padded window rows) may not be issued at all, so each wave counts the stores it certainly issued
//     (wave-uniform ballot) and picks the wait for that count: N is never larger than the number of younger operations.
// LDS: 3 x (24 + 16) KB + 5 x 2 KB of index = 130 KB, one 512-thread workgroup per CU.  No scratch: a spill would be a VMEM operation
// the counts do not know about (tests/test_rw_pipeline_no_scratch.py).
#include "common.h"

#include <utility>
#include "gemm_epilogue.h"

#ifdef SWV2_RW_STAMPS
__device__ unsigned long long rw_stamps[256 * 8];       // the qkv body
__device__ unsigned long long rw_dx_stamps[256 * 8];    // the streaming dx body
#define SWV2_STAMPS
#endif
#include "stamps.h"

namespace {

// LDS-DMA with a 64-bit per-lane source address (rows found through an index table: the tensor's size is not known to the selector)
__device__ __forceinline__ void dma_x4_va(const void* addr, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(addr), "s"(lds_addr) : "memory");
}
// one dword per lane to LDS at m0 + 4 * lane
__device__ __forceinline__ void dma_x1(const void* base, uint32_t byte_off, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" : : "v"(byte_off), "s"(base), "s"(lds_addr) : "memory");
}

struct RwDxEpi {            // what Epi<E_F32> carries for this product
    float* out;
    const float* bias;      // [128] or null
    const float* aux;       // residual rows, pitch ld
    const int32_t* rowidx;  // scatter table: logical row -> destination row, < 0 = skip
    long ld;
};

#ifndef SWV2_RW_SLOTS       // (A/B builds: 2 = one stage in flight)
#define SWV2_RW_SLOTS 3
#endif
constexpr int RW_NS = SWV2_RW_SLOTS;      // stage slots; RW_NS - 1 stages in flight

template <int NW>
__device__ __forceinline__ void rw_wait(int extra) {       // s_waitcnt vmcnt(NW + extra), extra in 0 .. 4: two stores in each of two stages
    static_assert(RW_NS == 2 || RW_NS == 3, "one case per possible store count");
    switch (extra) {
        case 0: asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW) : "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW + 1) : "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW + 2) : "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW + 3) : "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW + 4) : "memory"); break;
    }
}

// template arguments as the qkv body's (loader, epilogue, N, K, rows per stage, head slot): the kernel keeps its name for the profiles
template <int AK, int EK, int N, int K, int BMT, int HS = 16>
__global__ __launch_bounds__(512) void gemm_rw_kernel(ALoad<AK> al, const uint16_t* __restrict__ Wb, RwDxEpi ep, int M) {
    static_assert(AK == A_HEADS && EK == 1 && N == 128 && K == 384 && BMT == 32, "the d(qkv) -> dx product at C = 128");
    constexpr int NS = RW_NS, D = NS - 1, NI = 2 * D + 1;
    constexpr int KS = K / 32;                               // MFMA k-steps
    constexpr int A_ST = BMT * K * 2, R_ST = BMT * N * 4, I_ST = 8 * 256;
    constexpr int NA = A_ST / 1024 / 8, NR = R_ST / 1024 / 8;      // DMA instructions per wave and stage: 3 + 2 (+ 1 index)
    constexpr int NLD = NA + NR + 1;
    constexpr int OFF_A = 0, OFF_R = NS * A_ST, OFF_I = OFF_R + NS * R_ST, SMEM = OFF_I + NI * I_ST;
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM];       // (ONE array: a second one can cost a vmcnt(0) per ds_read)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int T = (M + BMT - 1) / BMT, G = gridDim.x;
    const int nst = (int)blockIdx.x < T ? (T - (int)blockIdx.x + G - 1) / G : 0;      // stages blockIdx.x, + G, ...
    if (nst == 0) return;
    auto stage_of = [&](int i) { return (int)blockIdx.x + min(i, nst - 1) * G; };       // (past the end: the last stage again, never consumed)
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    int* const idx_l = (int*)(smem + OFF_I);

    // ---- once: this wave's B fragments (columns 16 wave + fr), its bias value, the scatter entries of the first D stages
    bf16x8 bw[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bw[ks] = *(const bf16x8*)(Wb + (long)(16 * wave + fr) * K + ks * 32 + g * 8);
    const float bias = ep.bias ? ep.bias[16 * wave + fr] : 0.f;
    uint32_t acol[NA];                                       // element offset of (row 0, column block wave + 8 q)
#pragma unroll
    for (int q = 0; q < NA; ++q) acol[q] = al.elem_off(0, (wave + 8 * q) * 16);
#pragma unroll
    for (int d = 0; d < D; ++d)
        idx_l[(d % NI) * (I_ST / 4) + wave * 64 + lane] = ep.rowidx[min(stage_of(d) * BMT + 4 * wave + (lane >> 4), M - 1)];
    // the one-time loads are waited for HERE: a wait of the compiler's inside the loop would be a vmcnt(0) per stage
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : : "v"(bw[ks]));
    asm volatile("" : : "v"(bias), "v"(acol[0]), "v"(acol[NA - 1]));
    __syncthreads();                                         // (no DMA in flight yet: the compiler's own waits are exact up to here)

    // stage index i: A rows + residual rows into slot i % NS, the scatter entries of stage i + D into index slot (i + D) % NI
    auto issue = [&](int i) {
        const int s = stage_of(i), slot = i % NS;
        {
            const int m = min(s * BMT + (lane >> 1), M - 1);
            const uint32_t rowb = 2u * al.elem_off(m, 0) + (uint32_t)(lane & 1) * 16u;
#pragma unroll
            for (int q = 0; q < NA; ++q) dma_x4(al.d.ptr, rowb + 2u * acol[q], lds0 + OFF_A + slot * A_ST + (wave + 8 * q) * 1024);
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int r = 4 * wave + 2 * q + (lane >> 5);
            const int dst = max(idx_l[(i % NI) * (I_ST / 4) + wave * 64 + (2 * q + (lane >> 5)) * 16], 0);
            const int piece = (lane & 31) ^ ((wave & 1) << 2);                          // ((r >> 2) & 1) == wave & 1
            dma_x4_va(ep.aux + (long)dst * ep.ld + piece * 4, lds0 + OFF_R + slot * R_ST + (r & ~1) * 512);
        }
        {
            const int m = min(stage_of(i + D) * BMT + 4 * wave + (lane >> 4), M - 1);
            dma_x1(ep.rowidx, (uint32_t)m * 4u, lds0 + OFF_I + ((i + D) % NI) * I_ST + wave * 256);
        }
    };

    STAMP_DECL(8)
    STAMP_START();
#pragma unroll
    for (int d = 0; d < D; ++d) issue(d);
    int st1 = 0, st2 = 0;                                    // stores this wave certainly issued in the last / the last but one stage
    for (int t = 0; t < nst; ++t) {
        // the DMAs of stage t are older than (D - 1) stages of DMAs and the row stores of the last D stages
        rw_wait<(D - 1) * NLD>(__builtin_amdgcn_readfirstlane(D == 1 ? st1 : st1 + st2));
        STAMP(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();                        // stage t has landed (every wave's part); every wave is done with stage t - 1
        __builtin_amdgcn_sched_barrier(0);
        STAMP(1);
        issue(t + D);
        __builtin_amdgcn_sched_barrier(0);
        STAMP(2);
        const int s = stage_of(t), slot = t % NS;
        const unsigned char* As = smem + OFF_A + slot * A_ST;
        float* Rs = (float*)(smem + OFF_R + slot * R_ST);
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bf16x8 af = *(const bf16x8*)(As + (2 * ks + (g >> 1)) * 1024 + (16 * i + fr) * 32 + (g & 1) * 16);
                acc[i] = mfma32(af, bw[ks], acc[i]);
            }
        STAMP_DEP(3, acc[1][3]);
        // (acc + bias) + residual, in place: rows 16 i + 4 g + e, column 16 wave + fr
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 16 * i + 4 * g + e;
                float* p = Rs + row * N + (((4 * wave + (fr >> 2)) ^ ((g & 1) << 2)) << 2) + (fr & 3);       // ((row >> 2) & 1) == g & 1
                *p = (acc[i][e] + bias) + *p;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        STAMP(4);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();                        // every column of the stage's rows is in the tile
        __builtin_amdgcn_sched_barrier(0);
        STAMP(5);
        int issued = 0;
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int r = 4 * wave + 2 * q + (lane >> 5);
            const int dst = idx_l[(t % NI) * (I_ST / 4) + wave * 64 + (2 * q + (lane >> 5)) * 16];
            const bool valid = dst >= 0 && s * BMT + r < M;
            const f32x4 v = *(const f32x4*)(Rs + r * N + (lane & 31) * 4);
            const int piece = (lane & 31) ^ ((wave & 1) << 2);
            if (valid) *(f32x4*)(ep.out + (long)dst * ep.ld + piece * 4) = v;
            issued += __ballot(valid) != 0ull;
        }
        st2 = st1;
        st1 = issued;
        STAMP(6);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the re-issued tail stages still write this workgroup's LDS
#ifdef SWV2_RW_STAMPS
    if (tid == 0)
        for (int k = 0; k < 8; ++k) rw_dx_stamps[blockIdx.x * 8 + k] = st_acc[k];
#endif
}

// ------------------------------------------------------------------------------------------------
// Resident-weight kernel for the qkv product of a block at the benchmark width (N = 384, K = 128; N = 256, K = 192 per q / k / v part at
// C = 192).  The block's other row-streaming product, d(qkv) -> dx (N = 128, K = 384), started on this body and now runs the streaming
// body above (weight in registers, rows by LDS-DMA).  gemm_nt_kernel (gemm.hip) is latency-bound there (measured: ~20 us workgroup lifetime for
// 64 rows = one HBM round trip for the A panel + six dependent L2 round trips for the weight tiles + three epilogues, at
// three workgroups per CU -> 3 TB/s).  Here ONE persistent 8-wave workgroup per CU keeps the whole bf16 weight (96 KB) in
// LDS, walks row tiles t = blockIdx.x, + gridDim.x, ... and always has the NEXT tile's A rows in flight in registers while
// the current tile runs its MFMAs and its epilogue: per tile one A commit, no weight traffic, two barriers.
//   LDS: W[N][K] (swizzled 16-byte chunks) | A tile [BMT][K] bf16, re-used as the waves' epilogue staging
//   waves: 4 row groups x 2 column halves; wave tile = (BMT / 4) x (N / 2)
// ------------------------------------------------------------------------------------------------
// swizzled element offset of chunk kc of row r in a [rows][K] bf16 tile
__device__ __forceinline__ int swzk(int r, int kc, int K) { return r * K + (swz_chunk(r, kc) << 3); }

template <int AK, int EK, int N, int K, int BMT, int HS = 16>
__global__ __launch_bounds__(512) void gemm_rw_kernel(ALoad<AK> al, const uint16_t* __restrict__ Wb, Epi<EK> ep, int M) {
    constexpr int NTH = 512, KC = K / 8;                    // 16-byte chunks per row
    constexpr int ACH = BMT * KC / NTH;                     // A chunks per thread per tile
    constexpr int RT = BMT / 64;                            // 16-row MFMA tiles per wave (4 row groups)
    constexpr int CT = N / 32;                              // 16-column MFMA tiles per wave (2 column halves)
    constexpr int WCH = N * KC / NTH;                       // weight chunks per thread (one-time load)
    constexpr int A_BYTES = BMT * K * 2, ST_BYTES = 8 * 16 * EP * 4;
    constexpr int AS_BYTES = A_BYTES > ST_BYTES ? A_BYTES : ST_BYTES;
    static_assert(BMT * KC % NTH == 0 && N * KC % NTH == 0 && K % 64 == 0 && N % 64 == 0, "tile shapes");
    static_assert(N * K * 2 + AS_BYTES <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) uint16_t Ws[N * K];
    __shared__ __attribute__((aligned(16))) unsigned char as_raw[AS_BYTES];
    // The epilogue must not LOAD from global memory: such a load sits behind the next tile's A prefetch in the in-order
    // vmcnt queue, so waiting for it exposes the whole HBM round trip of the prefetch right there (measured with the
    // generic Epi::tile: 52 % / 40 % of the kernel inside the epilogue, 6 % in the explicit wait for A).  The bias lives
    // in LDS.
    __shared__ __attribute__((aligned(16))) float bs[N];
    uint16_t* As = (uint16_t*)as_raw;
    float* stage_all = (float*)as_raw;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int ntiles = (M + BMT - 1) / BMT;
    static_assert(AK == A_F32 && EK == E_QKV_HEADS, "instantiated for the qkv product only");
    for (int i = tid; i < N; i += NTH) bs[i] = ep.d.bias ? ep.d.bias[i] : 0.f;

    // ONE tile of A rows in flight per workgroup in registers.  (Two sets used alternately were measured SLOWER, 60.5 vs
    // 54.1 us for qkv: the kernel is not short of outstanding bytes.)  The gather rows of tile t + 2G are resolved while
    // tile t + G's data loads are issued, so the index load is never in front of a data load.
    typename ALoad<AK>::Raw ra[ACH];
    int arow[ACH];
    // chunk c of a tile -> (row, 16-byte chunk column): consecutive threads walk a row
    auto crow = [&](int c) { return c / KC; };
    auto ccol = [&](int c) { return c % KC; };
    // Every load of the staging pipeline is UNCONDITIONAL (clamped address); validity travels in bit masks and invalid
    // chunks (rows past M, padded window rows) are zeroed when the tile is written to LDS.  Loads under `if` made the
    // compiler guard their destination registers with s_waitcnt vmcnt(0) right behind them, which turned the prefetch into
    // a synchronous load (see gemm_tn.hip).  The launcher guarantees the gather table this kernel reads unconditionally.
    uint32_t ain = 0;                 // bit i: chunk row i of the next issue lies inside [0, M)
    uint32_t aok = 0;                 // chunks in flight: bit i = valid
    auto resolve = [&](int t) {
        ain = 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int c = tid + i * NTH, m = t * BMT + crow(c);
            const bool in = (t < ntiles) && (m < M);
            ain |= (uint32_t)in << i;
            arow[i] = al.d.rowidx[min(m, M - 1)];           // gather table entry (may be -1: padded row)
        }
    };
    auto issue = [&]() {
        aok = 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int c = tid + i * NTH;
            const int r = ((ain >> i) & 1) ? arow[i] : -1;
            ra[i] = al.raw_unc(max(r, 0), ccol(c) * 8);     // (unconditional: 47.9 -> 44.6 us against the load under `if`)
            aok |= (uint32_t)(r >= 0) << i;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int c = tid + i * NTH;
            *(uint4*)(As + swzk(crow(c), ccol(c), K)) = ((aok >> i) & 1) ? al.cvt(ra[i]) : make_uint4(0, 0, 0, 0);
        }
    };
    const int G = gridDim.x;
    STAMP_DECL(8)
    auto tile_step = [&](int t) {
        STAMP_WAITV();
        STAMP(0);
        commit();
        STAMP(1);
        __syncthreads();                                   // A tile (and, the first time, the weight) visible
        STAMP(2);
        issue();                                           // next tile's rows: in flight during the MFMAs and the epilogue
        resolve(t + 2 * G);
        STAMP(3);
        f32x4 acc[RT][CT];
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < CT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < K / 32; ++ks) {
            bf16x8 af[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) af[i] = *(const bf16x8*)(As + swzk(wr * 16 * RT + i * 16 + fr, ks * 4 + g, K));
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const bf16x8 bf = *(const bf16x8*)(Ws + swzk(wc * (N / 2) + j * 16 + fr, ks * 4 + g, K));
#pragma unroll
                for (int i = 0; i < RT; ++i) acc[i][j] = mfma32(af[i], bf, acc[i][j]);
            }
        }
        asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[RT - 1][CT - 1][3]));
        STAMP(4);
        __syncthreads();                                   // every wave is done with the A tile: it becomes the staging area
        STAMP(5);
        float* st = stage_all + wave * 16 * EP;
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j0 = 0; j0 < CT; j0 += 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[(4 * g + r) * EP + 16 * j + fr] = acc[i][j0 + j][r];
                const int m0 = t * BMT + wr * 16 * RT + i * 16, n0 = wc * (N / 2) + j0 * 16;
                {
                    // What heads_item<HS, true> computes, with the bias from LDS and all 64 lanes at work: lane = (row r, 16-column
                    // slot); HS = 32: a head is two slots (adjacent lane groups share the squared norm).  d.p1 = first q / k / v part
                    // of this launch's columns (a launch over one part of a split weight: BASELINE configs[4], see swv2_rw_qkv_launch)
                    const EpiDesc& d = ep.d;
                    const HeadLayout l = epi_layout(d, 3, HS);
                    const int L = d.p4;
                    const int r = lane & 15, slot = lane >> 4, nb = n0 + slot * 16, m = m0 + r;
                    if (m < d.M) {
                        const HeadLayout::Col c = l.col_of(HS == 16 ? nb >> 4 : nb >> 5, nb);
                        const int hd = c.hd, part = c.part + d.p1;
                        const HeadLayout::Row rw = l.row(m);
                        const int bw = rw.bw, tt = rw.t;
                        const bool valid = tt < L;
                        float v[16];
                        float ss = 0.f;
#pragma unroll
                        for (int j = 0; j < 16; j += 4) {
                            const f32x4 x = *(const f32x4*)(st + r * EP + slot * 16 + j) + *(const f32x4*)(bs + nb + j);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v[j + e] = valid ? x[e] : 0.f;
                                ss = fmaf(v[j + e], v[j + e], ss);
                            }
                        }
                        if constexpr (HS == 32) ss += __shfl_xor(ss, 16);      // (rows m and m past d.M differ only in lane bits 0 .. 3)
                        float rn = 1.f;
                        if (part < 2) {
                            rn = 1.f / fmaxf(sqrtf(ss), 1e-12f);
                            if (HS == 16 || !(slot & 1)) d.aux_out[l.rnorm_off(bw, hd, part, tt)] = valid ? rn : 0.f;
                        }
                        uint16_t* o = (uint16_t*)d.out + l.off(bw, hd, part, tt) + (HS == 32 ? (slot & 1) * 16 : 0);
                        float w8[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) w8[e] = v[e] * rn;
                        *(uint4*)o = pack8(w8);
#pragma unroll
                        for (int e = 0; e < 8; ++e) w8[e] = v[8 + e] * rn;
                        *(uint4*)(o + 8) = pack8(w8);
                    }
                }
            }
        STAMP(6);
        __syncthreads();                                   // staging consumed before the next commit overwrites it
        STAMP(7);
    };
    int t = blockIdx.x;
    resolve(t);
    issue();                                               // first tile's rows in flight before the weight is fetched
    resolve(t + G);
    // ---- the weight, once (made visible by the first tile's barrier)
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int c = tid + i * NTH, n = c / KC, kc = c - n * KC;
        *(uint4*)(Ws + swzk(n, kc, K)) = *(const uint4*)(Wb + (long)n * K + kc * 8);
    }

    STAMP_START();
    for (; t < ntiles; t += G) tile_step(t);
#ifdef SWV2_RW_STAMPS
    if (tid == 0)
        for (int k = 0; k < 8; ++k) rw_stamps[blockIdx.x * 8 + k] = st_acc[k];
#endif
}

}  // namespace

// gemm.hip (launch_nt2, LinearKernel::RESIDENT_QKV128 / RESIDENT_QKV192X3): the selector has checked the shape, the head slots and the gather table
int swv2_rw_qkv_launch(int parts, const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, hipStream_t st) {
    const uint16_t* wb = (const uint16_t*)w;
    if (parts == 1) {
        Epi<E_QKV_HEADS> ep = make_epi<E_QKV_HEADS>(e, M, 384);
        ep.d.p1 = 0;                                      // (first part of the launch's columns; p[1] is not a parameter of this epilogue)
        hipLaunchKernelGGL((gemm_rw_kernel<A_F32, E_QKV_HEADS, 384, 128, 128>), dim3(256), dim3(512), 0, st, make_loader<A_F32>(a), wb, ep, M);
        return SWV2_OK;
    }
    for (int part = 0; part < 3; ++part) {
        Epi<E_QKV_HEADS> ep = make_epi<E_QKV_HEADS>(e, M, 256);
        ep.d.p1 = part;
        ep.d.bias = e->bias ? e->bias + 256 * part : nullptr;
        hipLaunchKernelGGL((gemm_rw_kernel<A_F32, E_QKV_HEADS, 256, 192, 128, 32>), dim3(256), dim3(512), 0, st, make_loader<A_F32>(a),
                           wb + (size_t)part * 256 * 192, ep, M);
    }
    return SWV2_OK;
}
// gemm.hip (launch_nt2, LinearKernel::RESIDENT_DX128): the selector has checked the shape, both tables and the operand's 32-bit byte offsets
int swv2_rw_dx128_launch(const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, hipStream_t st) {
    RwDxEpi ep = {(float*)e->out, (const float*)e->bias, (const float*)e->aux, (const int32_t*)e->rowidx, e->ld};
    hipLaunchKernelGGL((gemm_rw_kernel<A_HEADS, 1, 128, 384, 32>), dim3(256), dim3(512), 0, st, make_loader<A_HEADS>(a), (const uint16_t*)w, ep, M);
    return SWV2_OK;
}

#ifdef SWV2_RW_STAMPS
extern "C" int swv2_debug_rw_stamps(void* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(rw_stamps), sizeof(unsigned long long) * 256 * 8) == hipSuccess ? 0 : -3;
}
extern "C" int swv2_debug_rw_dx_stamps(void* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(rw_dx_stamps), sizeof(unsigned long long) * 256 * 8) == hipSuccess ? 0 : -3;
}
#endif
