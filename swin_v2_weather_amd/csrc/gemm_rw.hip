// Streaming body of the resident-weight row GEMM for a block's d(qkv) -> dx product at C = 128 (N = 128, K = 384, gfx950 / CDNA4):
//   dx[rowidx[m]][0..127] = (dqkv[m][0..383] . W^T + bias) + residual[rowidx[m]][0..127]
// gemm.hip's first body of gemm_rw_kernel keeps the weight in LDS and runs its phases in series per row tile (wait for the register-
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
#include "gemm_common.h"

#ifdef SWV2_RW_STAMPS
__device__ unsigned long long rw_dx_stamps[256 * 8];
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

// template arguments as the first body's (loader, epilogue, N, K, rows per stage, head slot): the kernel keeps its name for the profiles
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

}  // namespace

// gemm.hip (launch_nt2, LinearKernel::RESIDENT_DX128): the selector has checked the shape, both tables and the operand's 32-bit byte offsets
int swv2_rw_dx128_launch(const swv2_operand* a, const void* w, const swv2_epilogue* e, int M, hipStream_t st) {
    RwDxEpi ep = {(float*)e->out, (const float*)e->bias, (const float*)e->aux, (const int32_t*)e->rowidx, e->ld};
    hipLaunchKernelGGL((gemm_rw_kernel<A_HEADS, 1, 128, 384, 32>), dim3(256), dim3(512), 0, st, make_loader<A_HEADS>(a), (const uint16_t*)w, ep, M);
    return SWV2_OK;
}

#ifdef SWV2_RW_STAMPS
extern "C" int swv2_debug_rw_dx_stamps(void* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(rw_dx_stamps), sizeof(unsigned long long) * 256 * 8) == hipSuccess ? 0 : -3;
}
#endif
