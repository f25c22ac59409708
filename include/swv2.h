/* swv2 -- C ABI of the MI355X-native SwinV2 weather hot path (libswv2.so).
 *
 * The reference (NERSC/swin_v2_weather, 100 % Python) has no FFI boundary: its hot path is the PyTorch op sequence
 * inside networks/swinv2_global.py.  This header is the boundary a maintainer binds instead (ctypes stub in
 * INTEGRATION.md): each entry point replaces the op sequence cited next to it.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, explicit sizes, no torch types.  `stream` is a hipStream_t passed as void*
 *    (0 = the null stream); every call only enqueues work on that stream and returns.
 *  - every function returns SWV2_OK (0) or a negative error code and never throws; `swv2_last_error()` returns a
 *    thread-local message for the last failure on the calling thread.
 *  - no entry point allocates, frees or synchronises: the caller owns all memory, including workspaces, so every
 *    call can be captured in a hipGraph.
 *  - no hidden global device state: re-entrant from autograd worker threads.
 *  - dtypes: activations that cross kernels are bf16 (uint16 storage) unless stated; the residual stream, LayerNorm
 *    statistics, log-sum-exp and all parameter gradients are fp32.  MFMA products take bf16 operands and
 *    accumulate in fp32.
 */
#ifndef SWV2_H
#define SWV2_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision: bumped whenever a struct layout or an entry point of this header changes (swv2_version() returns the value the
 * library was built with; swin_v2_weather_amd/_lib.py refuses a library whose revision differs from the one it mirrors).
 * 100 rounds 1 - 4; 105 round 5: swv2_attn_args.dbias_partials, swv2_block_desc.bias_prepacked / dbias_part, the *_multi CPB
 * entry points, swv2_attn_pack_bias_multi / swv2_attn_bias_chunks, a (max, min) part in the packed bias buffer;
 * 106: SWV2_EPI_UNPATCH_LOSS writes slot 1 of loss_part only where swv2_loss_part_reduce reads it; 107: swv2_epilogue.q[3], the loss
 * epilogue with the rollout destinations; 108: the kernel-selection queries swv2_linear_kernel, swv2_linear_wgrad_kernel,
 * swv2_block_wgrad_kernel; 109: swv2_block_plan (+ swv2_block_plan_t, enum swv2_block_step, swv2_block_step_id / _name),
 * swv2_block_desc loses fuse_attn and wgrad_side_stream; 110: the attention kernel-selection queries swv2_attn_fwd_kernel /
 * swv2_attn_bwd_kernel (+ swv2_attn_kernel_t, SWV2_ATTN_K_*); 111: the LAMB optimizer, swv2_lamb_* (+ swv2_lamb_item, SWV2_LAMB_*);
 * 112: forecast scores, swv2_score_*.  The dataset statistics, swv2_stats_*, came later and are purely additive (new entry points only,
 * no struct member moves): the revision stays 112.  So are the plane order statistics, swv2_quantile_ws_bytes / swv2_plane_order_stats,
 * and the ensemble scores, swv2_ens_*, and the l1 loss family, swv2_l1_*, and the spherical-harmonic degree spectra, swv2_sht_*;
 * 113: swv2_loss_sums takes a workspace (+ swv2_loss_ws_bytes) and no longer needs zeroed sums. */
#define SWV2_VERSION 113

enum {
    SWV2_OK = 0,
    SWV2_ERR_INVALID = -1,     /* bad argument (null pointer, size, alignment) */
    SWV2_ERR_UNSUPPORTED = -2, /* shape outside the compiled kernel set */
    SWV2_ERR_LAUNCH = -3       /* HIP launch failure */
};

int swv2_version(void);
const char* swv2_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Window-ordered, head-major attention layout (produced by swv2_linear with SWV2_EPI_QKV_HEADS):
 *   qkvh  [Bw][heads][3][Lp][DP] bf16   s=0: q/max(|q|,1e-12)  s=1: k/max(|k|,1e-12)  s=2: v ; zero padded
 *   rnorm [Bw][heads][2][Lp]     fp32   1/max(|q|,1e-12), 1/max(|k|,1e-12)
 *   oh    [Bw][heads][Lp][DP]    bf16   attention output, heads not yet merged
 *   lse   [Bw][heads][Lp]        fp32   log2-domain log-sum-exp of the scaled, biased, masked scores
 * Bw = B * windows per sample, window index = b*nW + wi*nww + wj, token index t = r*ww + c
 * (reference: window_partition, swinv2_global.py:89-101).  Lp, DP: swv2_attn_geometry().
 * Padding contract, the same for every kernel family (checked element by element in tests/test_attn_exact_gpu.py):
 *   inputs : rows >= L and columns >= head_dim of qkvh and doh are zero, rows >= L of rnorm are zero (the qkv epilogue and
 *            swv2_proj_ln_bwd / the d(oh) product leave them so); the kernels read them.
 *   oh     : rows >= L and columns >= head_dim are written as exactly 0 by the forward.
 *   lse    : rows >= L are written as exactly 0.
 *   dqkvh  : rows >= L of all three parts (dq, dk, dv) are written as exactly 0 -- the weight-gradient kernels sum over all Lp rows and
 *            rely on it; columns >= head_dim of rows < L are UNSPECIFIED (a caller must not read them; the qkv weight gradient drops them
 *            through its column map).
 *   dlogit_scale, dbias: only the [heads] / [heads][L][L] elements are touched; a head with tau > ln 100 adds exactly 0.
 * ------------------------------------------------------------------------------------------------------------ */
int swv2_attn_geometry(int L, int head_dim, int* Lp, int* DP);

/* Which forward softmax regime serves window area L / head_dim (with / without a PACKED CPB bias table; dbg as in swv2_attn_args): 1 = the
 * operand-folded softmax of csrc/attn2.hip (160 .. 176-token windows; 16- and 32-wide head slots without a table, 16-wide ones with
 * a packed table; exponent reference sigma' (+ the table's maximum) where 2 sigma' + (table max - min) <= 80 in unmasked windows,
 * normaliser = sum of the bf16-rounded exponentials), 0 = row maximum + exact sum (csrc/attn.hip, attn_wide.hip); negative: unsupported geometry.
 * Pure host function; the `regime` field of swv2_attn_fwd_kernel's answer for the same geometry.  It speaks of a head WIDTH, not of one launch: at
 * head_dim 256, which has no table form, it answers 0 whatever has_bias says, while swv2_attn_fwd_kernel refuses a table there.  The parity tests declare the regime their oracle emulates and check it against this (reference: the softmax of
 * swinv2_global.py:309-314, one function in both regimes up to rounding). */
int swv2_attn_fwd_regime(int L, int head_dim, int has_bias, int dbg);

#define SWV2_ATTN_FIRST_GEN 16
#define SWV2_ATTN_PLAIN_STATS 8192
#define SWV2_ATTN_BWD_TWO_PHASE 32

typedef struct swv2_attn_args {
    const void* qkvh;         /* in  */
    const float* logit_scale; /* in  [heads] raw tau; sigma = exp(min(tau, ln 100))   (swinv2_global.py:305) */
    const float* bias;        /* in  [heads][L][L] continuous position bias (swinv2_global.py:274-287) or NULL */
    const void* bias_pack;    /* optional: the same table pre-packed by swv2_attn_pack_bias (kernel register / LDS-image
                                 layouts, coalesced loads); NULL = the kernels convert `bias` themselves */
    void* oh;                 /* fwd: out; bwd: in */
    float* lse;               /* fwd: out; bwd: in */
    const void* doh;          /* bwd in : grad of oh, same layout */
    const float* rnorm;       /* bwd in */
    void* dqkvh;              /* bwd out: grads w.r.t. the un-normalised q, k, v, layout of qkvh */
    float* dlogit_scale;      /* bwd out: [heads], ACCUMULATED (caller zeroes) */
    float* dbias;             /* bwd out: [heads][L][L], ACCUMULATED (caller zeroes); NULL iff bias is NULL */
    int Bw, heads, L, head_dim;
    int nwh, nww;             /* windows per sample along H and W */
    int mask_thr;             /* shift mask (swinv2_global.py:403-424) in closed form: in the last window row
                                 (wi == nwh-1) tokens t >= mask_thr are region 1, others region 0; pairs from
                                 different regions get -100.  (wh - sh) * ww for a block shifted by sh > 0 rows;
                                 0 = no mask. */
    int max_chunks;           /* workgroups per head (each loops over windows); 64 is a good default (swv2_block_bwd uses
                                 256 / heads at the 176-token window: one persistent workgroup per CU) */
    int dbg;                  /* 0 in production.  Kernel-selection switches used by the parity tests (each selects a kernel that is
                                 also the product path of other shapes): SWV2_ATTN_FIRST_GEN = the first-generation kernels of
                                 csrc/attn.hip instead of the small-workgroup forward of csrc/attn2.hip; SWV2_ATTN_PLAIN_STATS =
                                 the two-phase backward with the softmax statistics read from LDS instead of riding in the
                                 MFMA operands; SWV2_ATTN_BWD_TWO_PHASE = the barrier-separated two-phase backward of csrc/attn.hip
                                 (statistics in the operands) where csrc/attn_bwd_stream.hip would run (176-row layout, 16-wide
                                 head slots, no table): same arithmetic, bit-identical d(qkv).  None applies at head_dim 256:
                                 csrc/attn_d256.hip is the only kernel pair there */
    void* dbias_ws;           /* bwd, optional scratch of dbias_ws_bytes >= swv2_attn_dbias_ws_bytes(heads, L, max_chunks): the
                                 workgroups store their d bias tables there and one more launch sums them into dbias (in a
                                 fixed order); NULL / too small = 31 K float atomics per workgroup instead */
    size_t dbias_ws_bytes;
    int dbias_partials;       /* bwd, 1 (needs dbias_ws): LEAVE the workgroups' tables in dbias_ws -- [swv2_attn_bias_chunks(Bw)][heads][L][L],
                                 every entry written -- and do not touch dbias (may be NULL): the caller sums them, e.g. swv2_cpb_bwd_multi */
} swv2_attn_args;

/* Which kernel swv2_attn_fwd / swv2_attn_bwd launch for these arguments: the family (SWV2_ATTN_K_*, also the return value) and the
 * template arguments of the instantiation, or a negative error for a geometry no kernel serves (head_dim 129 .. 255, head_dim 256 with
 * a table or in the 64-row layout, L > 176).  Pure host functions: they read L, head_dim, dbg and the PRESENCE of bias / bias_pack,
 * dereference no pointer, launch nothing and need no GPU (`out` may be NULL).  The launchers switch on the same selection function,
 * and the tests assert on this answer where they name a path. */
#define SWV2_ATTN_K_D256 0       /* csrc/attn_d256.hip: 256-channel heads, 176-row layout, no table                                  */
#define SWV2_ATTN_K_FWD3 1       /* csrc/attn2.hip: operand-folded forward, 16-wide slots, 160 .. 176 tokens, no table              */
#define SWV2_ATTN_K_FWD3W 2      /* the same at 32-wide slots                                                                       */
#define SWV2_ATTN_K_FWD3B 3      /* the same at 16-wide slots with a PACKED table                                                   */
#define SWV2_ATTN_K_WIDE 4       /* csrc/attn_wide.hip: 65 .. 96 channels, 176-row layout, no table                                 */
#define SWV2_ATTN_K_STREAM 5     /* csrc/attn_bwd_stream.hip: streamed-dQ backward, 176-row layout, 16-wide slots, no table         */
#define SWV2_ATTN_K_FIRST_GEN 6  /* csrc/attn.hip: attn_fwd_kernel / attn_bwd_kernel<LT, DK, bias, LFIX>                            */
typedef struct swv2_attn_kernel_t {
    int family;              /* SWV2_ATTN_K_* */
    int Lp, DP;              /* swv2_attn_geometry */
    int LT, DK;              /* Lp / 16, DP / 16: the layout's row and column tiles */
    int LFIX;                /* the window area the instantiation is specialised for, 0 = the run-time-L one */
    int regime;              /* forward: swv2_attn_fwd_regime (1 = operand-folded softmax, normaliser = sum of the rounded exponentials) */
    /* backward, first generation (and `aug` of the streamed kernel): the compile-time variants that change arithmetic */
    int aug;                 /* softmax statistics, padded-key flag and shift mask ride in the MFMA operands (bf16 parts: lse and delta in
                                three, |error| <= 2^-24 |v|; the mask term -100 / sigma in two, <= 2^-17 of it) instead of fp32 from LDS */
    int bias_lds;            /* the table's image sits in LDS (else: rows in registers) */
    int qg;                  /* q / dO fragments are read from global memory */
} swv2_attn_kernel_t;
int swv2_attn_fwd_kernel(const swv2_attn_args* a, swv2_attn_kernel_t* out);
int swv2_attn_bwd_kernel(const swv2_attn_args* a, swv2_attn_kernel_t* out);

/* bytes of swv2_attn_args.dbias_ws for swv2_attn_bwd with a bias */
size_t swv2_attn_dbias_ws_bytes(int heads, int L, int max_chunks);

/* workgroups per head of swv2_attn_bwd with a bias table (= tables per head in dbias_ws) when max_chunks is left to swv2_block_bwd */
int swv2_attn_bias_chunks(int Bw);

/* bias table -> the kernels' layouts (bf16, log2 domain) + the (max, min) of every head's packed values; out:
 * swv2_attn_pack_bias_bytes(heads, L) bytes.  _multi: ntab tables [ntab][heads][L][L] -> ntab packed buffers, one launch */
size_t swv2_attn_pack_bias_bytes(int heads, int L);
int swv2_attn_pack_bias(const float* bias, int heads, int L, void* out, void* stream);
int swv2_attn_pack_bias_multi(const float* bias, int ntab, int heads, int L, void* out, void* stream);

/* cosine window attention core, forward: swinv2_global.py:304-318 (q,k normalisation is in the QKV epilogue) */
int swv2_attn_fwd(const swv2_attn_args* a, void* stream);
/* backward of the same, including the backward of the L2 normalisation of q and k */
int swv2_attn_bwd(const swv2_attn_args* a, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Linear layers: C[M][N] = A[M][K] . W[N][K]^T on bf16 MFMA with fp32 accumulation.
 * The A operand is described by a "loader" (what PyTorch does as separate passes in the reference is folded into
 * the load), the output by an "epilogue".  W is always bf16 [N][K] row-major, produced by swv2_prep_weight.
 * Replaces: nn.Linear / nn.Conv2d(k=s=4) + the layout ops around them in swinv2_global.py (qkv :300-301, proj :319,
 * Mlp fc1/fc2 :381-386, PatchEmbed.proj :537,544, PatchMerging :519-523, head + un-patchify :767,784-792).
 * ------------------------------------------------------------------------------------------------------------ */
enum swv2_operand_kind {
    SWV2_OP_F32 = 0,       /* fp32 rows [rows][ld]; optional rowidx gather (roll + window partition, :457,89-101)   */
    SWV2_OP_BF16 = 1,      /* bf16 rows [rows][ld]; optional rowidx gather                                          */
    SWV2_OP_BF16_GELU = 2, /* bf16 rows, erf-GELU applied on load (timm Mlp act)                                     */
    SWV2_OP_HEADS = 3,     /* head-major window layout [Bw][h][S][Lp][DP]: row = bw*Lp + t, col = (part*h+head)*DP+j
                              p[0]=heads p[2]=Lp p[3]=DP, ld = S                                                     */
    SWV2_OP_PATCH = 4,     /* im2col of x[B][Cin][H][W] fp32 for the 4x4/stride-4 conv: row=(b,i,j), col=cin*16+p*4+q
                              p[0]=Cin p[1]=H p[2]=W ; p[3] = channels per sample of the tensor holding the Cin planes
                              (0 = Cin) ; aux0 = optional second source added on load, ld = its channels per sample      */
    SWV2_OP_MERGE_LN = 5,  /* 2x2 PatchMerging gather of x[B][H][W][C] fp32 + LayerNorm(4C) on load:
                              p[0]=H p[1]=W p[2]=C, aux0=mean aux1=rstd (swv2_merge_stats) aux2=gamma aux3=beta     */
    SWV2_OP_BF16_CSCALE = 6 /* bf16 rows [rows][ld] scaled on load by an fp32 factor per (sample, group of 16 columns):
                              value = bf16(ptr[row][col] * aux0[(row / p[0]) * p[2] + col / 16]) ; p[0] = rows per sample,
                              p[2] = groups per sample in aux0.  The loss-gradient operand of the head's backward: ptr = the
                              quadrature-weighted residual written by SWV2_EPI_UNPATCH_LOSS, aux0 = d loss / d S0 per
                              (sample, channel) (losses.py:188-206).  Accepted by swv2_linear with SWV2_EPI_F32 and as dY of
                              swv2_linear_wgrad* with an SWV2_OP_F32 X                                              */
};

typedef struct swv2_operand {
    int kind;              /* enum swv2_operand_kind */
    const void* ptr;
    const int32_t* rowidx; /* optional: logical row -> source row, negative = all-zero row */
    const float* aux0;
    const float* aux1;
    const float* aux2;
    const float* aux3;
    long ld;               /* row pitch in elements (or S for SWV2_OP_HEADS) */
    int rows, cols;        /* logical M and K */
    int p[4];
} swv2_operand;

enum swv2_epilogue_kind {
    SWV2_EPI_BF16 = 0,      /* out bf16 [M][ld] = acc + bias ; optional rowidx scatter                               */
    SWV2_EPI_F32 = 1,       /* out fp32 [M][ld] = acc + bias (+ aux fp32, same shape, added at the destination
                               row: the residual gradient) ; optional rowidx scatter                                 */
    SWV2_EPI_QKV_HEADS = 2, /* out = qkvh, aux_out = rnorm: + bias, split heads, L2-normalise q and k (:300-304)
                               p[0]=heads p[2]=Lp p[3]=DP p[4]=L ; N = 3*heads*DP, bias padded alike                 */
    SWV2_EPI_GELU_GRAD = 3, /* out bf16 = acc * GELU'(aux) ; aux = bf16 pre-activation, same shape/pitch as out     */
    SWV2_EPI_UNPATCH = 4,   /* out fp32 y[B][Cout][H][W] (+ aux skip[B][Cs][H][W]) ; N = Cout*16 with columns ordered
                               c*16+p*4+q ; p[0]=Cout p[1]=H p[2]=W p[3]=Cs (0 = no skip)   (:784-802) ;
                               p[4] = channels per sample of the tensor `out` points into (0 = Cout) ; aux_out = optional
                               second destination, ld = its channels per sample (rollout, helpers.py:26-41)          */
    SWV2_EPI_HEADS = 5,     /* out = [Bw][h][Lp][DP] bf16 split heads, no normalisation ; p as QKV_HEADS, N=heads*DP */
    SWV2_EPI_F32_ACC = 6,   /* out fp32 [M][ld] += acc ; optional rowidx scatter                                     */
    SWV2_EPI_BF16_GELU = 7, /* out bf16 = acc + bias (pre-activation, kept for backward), aux_out bf16 = erf-GELU of it,
                               both [M][ld] (fc1 of the timm Mlp, swinv2_global.py:381-386)                         */
    SWV2_EPI_UNPATCH_LOSS = 8 /* SWV2_EPI_UNPATCH (single destination) that also evaluates the geometric l2 loss sums of
                               the prediction it is writing (losses.py:188-206, grids.py:115-117) against the target
                               loss_tar fp32 [B][q[0]][H][W] (channels q[1] .. q[1] + Cout): per (sample, channel)
                               sum_hw qw[h] (y - tar)^2 and sum_hw qw[h] tar^2, left as per-row-group partial sums
                               loss_part[g][slot][c][2] (g = group of SWV2_LOSS_GROUP_ROWS rows of the GEMM; slot 0 = rows of the sample of the
                               group's first row, slot 1 = rows of the following sample -- WRITTEN only by groups whose successor
                               row belongs to another sample or lies past M, the only groups swv2_loss_part_reduce reads it of;
                               zero there unless the group straddles the boundary; plain stores, no atomics: same-address float atomics from every workgroup
                               measured 8 x the whole kernel) which swv2_loss_part_reduce folds in a fixed order.  Also
                               writes loss_resid bf16 [M][SWV2_LOSS_RESID_PITCH(N)] = qw[h] (y - tar) in the GEMM's own row / column order -- the
                               operand SWV2_OP_BF16_CSCALE feeds to the head's backward, so neither the prediction nor a
                               materialised gradient is read again.  A operand: SWV2_OP_F32 only; at least
                               SWV2_LOSS_GROUP_ROWS rows per sample; every tensor below 2^32 elements; `out` and loss_resid must be
                               followed by SWV2_LOSS_DUMP_BYTES of write-only scratch (masked lanes store there, so that the
                               epilogue is branch-free).  Rollouts (107): p[4] = channels per sample of the tensor `out` points into
                               (with q[2]), aux_out / ld = a second destination [B][ld][H][W] for the same prediction (the next
                               step's input, also followed by SWV2_LOSS_DUMP_BYTES), as SWV2_EPI_UNPATCH has them  */
};

typedef struct swv2_epilogue {
    int kind;              /* enum swv2_epilogue_kind */
    void* out;
    const float* bias;     /* [N] or NULL */
    const void* aux;
    float* aux_out;
    const int32_t* rowidx; /* optional: logical row -> destination row, negative = skip */
    long ld;               /* output row pitch in elements */
    int p[5];
    /* SWV2_EPI_UNPATCH_LOSS only (ignored by every other kind) */
    const float* loss_tar;   /* target [B][q[0]][H][W] fp32 */
    const float* loss_qw;    /* quadrature row weights [H] */
    float* loss_part;        /* [ceil(M / SWV2_LOSS_GROUP_ROWS)][2][Cout][2] fp32 per-group partial sums: slot 0 overwritten, slot 1 see above */
    void* loss_resid;        /* bf16 [M][SWV2_LOSS_RESID_PITCH(N)], columns 0 .. N - 1 written */
    int q[3];                /* channels per sample of loss_tar, first target channel of this prediction, and (rollouts: p[4] != 0, `out`
                                points into a [B][p[4]][H][W] tensor) the offset in floats from `out` to that tensor's dump area; 0 = behind
                                the dense [B][Cout][H][W] prediction */
} swv2_epilogue;

int swv2_linear(const swv2_operand* a, const void* w_bf16, const swv2_epilogue* e, int N, void* stream);

/* Which kernel swv2_linear launches for these descriptors: one of SWV2_LINEAR_*, or a negative error for a kind pair it does not
 * serve.  Pure host function: reads the descriptors' kinds, sizes and p[], tests rowidx / aux for presence only, dereferences no data
 * pointer, launches nothing, needs no GPU.  The launcher switches on the same selection function, and the tests assert on this answer
 * where they name a path.  SWV2_GEMM_WIDE (environment, default 1; 0 = the tile kernels in place of the wide ones) is read per call. */
#define SWV2_LINEAR_RESIDENT_QKV128 0   /* resident-weight qkv product at C 128 (N 384, 16-wide head slots, gathered fp32 rows)          */
#define SWV2_LINEAR_RESIDENT_QKV192X3 1 /* the same at C 192 (N 768, 8 heads in 32-wide slots): three launches, one per q / k / v part */
#define SWV2_LINEAR_RESIDENT_DX128 2    /* resident-weight d(qkv) -> dx product at C 128 (N 128, K 384, residual add + scatter)        */
#define SWV2_LINEAR_WIDE_DMA 3          /* 256 x 256 tiles, operand staged by LDS-DMA (raw bf16 rows, head-major layouts)              */
#define SWV2_LINEAR_WIDE 4              /* 256 x 256 tiles, operand staged through registers (fp32 or gathered rows)                   */
#define SWV2_LINEAR_TILE64 5            /* 64-row x 128-column tiles                                                                   */
#define SWV2_LINEAR_TILE128 6           /* 128 x 128 tiles                                                                             */
int swv2_linear_kernel(const swv2_operand* a, const swv2_epilogue* e, int N);

/* Weight gradient: dW[nmap(n)][kmap(k)] += sum_m dY[m][n] X[m][k], db[nmap(n)] += sum_m dY[m][n]  (caller zeroes; db
 * may be NULL).  dW has row pitch ldw; nmap/kmap (NULL = identity, negative = drop) undo the head padding of the
 * SWV2_OP_HEADS layouts.  splits > 0 = number of row slices processed by different workgroups (x 2 for outputs of fewer
 * than three 128 x 128 tiles).  swv2_linear_wgrad sums the slices with fp32 atomics on dW; swv2_linear_wgrad_ws writes
 * per-slice partial tiles to the caller's workspace (>= swv2_linear_wgrad_ws_bytes(M, N, K, splits) bytes, contents
 * undefined afterwards) and adds them in a second kernel -- no atomics on dW, deterministic, and faster from ~64
 * slices up.  ws == NULL falls back to the atomic path.  Replaces the autograd of F.linear / Conv2d weights. */
int swv2_linear_wgrad(const swv2_operand* dy, const swv2_operand* x, float* dW, float* db, const int32_t* nmap,
                      const int32_t* kmap, int ldw, int splits, void* stream);
size_t swv2_linear_wgrad_ws_bytes(int M, int N, int K, int splits);
int swv2_linear_wgrad_ws(const swv2_operand* dy, const swv2_operand* x, float* dW, float* db, const int32_t* nmap,
                         const int32_t* kmap, int ldw, int splits, void* ws, size_t ws_bytes, void* stream);
/* Which kernel swv2_linear_wgrad_ws launches for operands the launcher accepts (ws_bytes = 0: no workspace, the atomic path of
 * swv2_linear_wgrad): SWV2_WGRAD_*, or a negative error.  Pure host function like swv2_linear_kernel; reads SWV2_GEMM_WIDE per call. */
#define SWV2_WGRAD_WIDE 0               /* 256 x 256 tiles by LDS-DMA, partial matrices in the workspace (N, K >= 512) */
#define SWV2_WGRAD_TILE 1               /* 128 x 128 tiles: atomics, or per-slice partial tiles in the workspace       */
int swv2_linear_wgrad_kernel(const swv2_operand* dy, const swv2_operand* x, int splits, size_t ws_bytes);

/* The four weight gradients of one transformer block in ONE launch + one reduction (item 0: fc2 = (BF16, BF16_GELU),
 * 1: fc1 = (BF16, F32), 2: proj = (BF16, HEADS), 3: qkv = (HEADS, F32); any other operand kinds -> SWV2_ERR_INVALID).
 * slices > 0, and slices = 0 at block shapes the slab kernel does not cover, run the 128 x 128 tile kernel: the results of
 * four swv2_linear_wgrad_ws calls up to the summation order of the row slices (count: slices; 0 = one round of 2 workgroups
 * per CU).  slices = 0 at the slab kernel's shapes (gemm_tn_slab.hip: C 128 / hidden 512 / 8 x 16 head columns, C 192 / 768 /
 * 8 x 32) runs one workgroup per CU, each rounding its partial dW tile to bf16 before the fp32 fold: per element
 * |dW - exact| <= 2^-8 sum_m |dY[m][n] X[m][k]| instead of the fp32 paths' ~1e-7 of it (bias gradients stay fp32).
 * ws >= swv2_block_wgrad_ws_bytes(C, hidden, heads * DP, slices) bytes.  Replaces: the autograd of the block's four
 * nn.Linear weights (swinv2_global.py:146-201, 231-248). */
typedef struct swv2_wgrad_item {
    swv2_operand dy, x;
    float* dW;
    float* db;             /* optional */
    const int32_t* nmap;
    const int32_t* kmap;
    int ldw;
} swv2_wgrad_item;
size_t swv2_block_wgrad_ws_bytes(int C, int hidden, int heads_dp, int slices);
int swv2_block_wgrad(const swv2_wgrad_item* items4, int slices, void* ws, size_t ws_bytes, void* stream);
/* Which kernel swv2_block_wgrad launches: SWV2_BLOCK_WGRAD_*, or a negative error.  Pure host function like swv2_linear_kernel.  The
 * slab kernel's plan depends on the CU count of the calling thread's current device; in a process without a GPU the answer is the one
 * for 256 CUs (the library's fallback count). */
#define SWV2_BLOCK_WGRAD_SLAB 0         /* gemm_tn_slab.hip: slices = 0 at its two block shapes with a workspace that holds its plan */
#define SWV2_BLOCK_WGRAD_GROUPED 1      /* the grouped 128 x 128 tile kernel                                                          */
int swv2_block_wgrad_kernel(const swv2_wgrad_item* items4, int slices, size_t ws_bytes);
/* The plan behind that answer, from the function swv2_block_wgrad itself switches on.  cus = 0: the calling thread's current device
 * (as swv2_block_wgrad_kernel); cus > 0: plan the slab kernel for that many CUs -- host arithmetic only, so a process without a GPU
 * can sweep it.  Per product (0 fc2, 1 fc1, 2 proj, 3 qkv): S row slices, SR rows per stage (slab: slice s owns the stages s, s + S,
 * ...; grouped: the 128-row steps of the tile kernel), the workgroups launched for it; bytes: the workspace the plan needs
 * (<= swv2_block_wgrad_ws_bytes).  Additive to revision 113 (a new entry point and its struct, no member of another struct moves). */
typedef struct swv2_block_wgrad_plan_t {
    int kernel;            /* SWV2_BLOCK_WGRAD_* */
    int S[4];
    int SR[4];
    int wgs[4];
    size_t bytes;
} swv2_block_wgrad_plan_t;
int swv2_block_wgrad_plan(const swv2_wgrad_item* items4, int slices, size_t ws_bytes, int cus, swv2_block_wgrad_plan_t* out);

/* Head dims 65 .. 128 (DP = 96 up to 96 channels, else 128): SWV2_EPI_QKV_HEADS then leaves the squared norms of q, k in rnorm (which the
 * caller zeroes first) and un-normalised values in qkvh; this pass finishes F.normalize (swinv2_global.py:300-304):
 * rnorm <- 1 / max(|.|, 1e-12) (0 on rows >= L) and q, k rescaled in place. */
int swv2_qk_normalize(void* qkvh_bf16, float* rnorm, int Bw, int heads, int Lp, int L, int DP, void* stream);

/* out_bf16[i][j] = W'[row_map ? row_map[i] : i][col_map ? col_map[j] : j] (0 where a map entry is negative),
 * W' = transpose ? w^T : w, w fp32 [rows][cols].  Casts, transposes, permutes and pads a parameter once per step. */
int swv2_prep_weight(const float* w, int rows, int cols, int transpose, const int32_t* row_map, int out_rows,
                     const int32_t* col_map, int out_cols, void* out_bf16, void* stream);

/* The same for many parameters in ONE launch (all prepared copies of a model after an optimizer step).  items_dev: device
 * array; chunks_dev: device array of int pairs (item index, chunk index within the item's output), one workgroup per chunk
 * of swv2_prep_chunk() output elements; both tables are built by the caller (swin_v2_weather_amd/ops.py::PrepBatch).
 * out_f32 != 0: the output stays fp32 (the head-padded qkv bias). */
typedef struct swv2_prep_item {
    const float* w;
    int rows, cols, transpose;
    const int32_t* row_map;
    int out_rows;
    const int32_t* col_map;
    int out_cols;
    void* out;
    int out_f32;
} swv2_prep_item;
int swv2_prep_chunk(void);
/* number of workgroups (chunk indices 0 .. n - 1 of the pair table) item needs: linear chunks of swv2_prep_chunk() outputs, or
 * 64 x 64 output tiles for transposed copies of matrices with both dimensions >= 64 (turned in LDS) */
int swv2_prep_item_chunks(int out_rows, int out_cols, int transpose);
int swv2_prep_multi(const swv2_prep_item* items_dev, const int* chunks_dev, int n_chunks, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused LayerNorm + drop-path + residual add, with the window_reverse + reverse cyclic roll folded into the row
 * scatter:  y[dst] = res[res_mod ? dst % res_mod : dst] + scale[dst / rows_per_sample] * (LN(a[m])*gamma + beta),
 * dst = rowidx ? rowidx[m] : m (negative = padded row, skipped).
 * The drop-path factor is scale[dst / rows_per_sample] of the DESTINATION row and nothing more: rows_per_sample need not divide M,
 * the rows of a window or any tile height.  mean / rstd are written for every row m, padded ones included (the statistics of
 * a[m] like any other row); only the y row is skipped, and y rows that no table entry names are not written.  The backward
 * reads a, mean, rstd of every row (they must be finite on padded rows too), writes da = +0 on padded rows and counts them in
 * neither dgamma nor dbeta.  Forward: 4096 workgroups at most, backward SWV2_LN_BWD_MAX_BLOCKS, then grid stride.
 * Per-element accuracy against fp64 of the saved tensors: tests/test_proj_ln_exact_gpu.py (bounds: tests/proj_ln_reference.py).
 * Replaces  x + drop_path(norm(branch))  (swinv2_global.py:490,496), window_reverse + roll (:468-476) and
 * PatchEmbed's norm + pos_embed add (:545,780 with res = pos_embed as [T][C], res_mod = T).
 * ------------------------------------------------------------------------------------------------------------ */
#define SWV2_LN_BWD_MAX_BLOCKS 512
typedef struct swv2_ln_args {
    const void* a;         /* bf16 [M][C] branch output                                   */
    const float* res;      /* fwd: fp32 residual rows (NULL = 0)                           */
    const float* gamma;    /* [C] */
    const float* beta;     /* [C] (fwd) */
    const float* scale;    /* [B] drop-path factor per sample or NULL                     */
    const int32_t* rowidx; /* [M] or NULL                                                  */
    float* y;              /* fwd out: fp32 rows                                           */
    float* mean;           /* [M] fwd: out, bwd: in */
    float* rstd;           /* [M] fwd: out, bwd: in */
    const float* dy;       /* bwd in : fp32 grad of y (destination rows)                  */
    void* da;              /* bwd out: bf16 [M][C] grad of a (zeros on padded rows)       */
    float* dgamma;         /* bwd out: [C] ACCUMULATED */
    float* dbeta;          /* bwd out: [C] ACCUMULATED */
    float* ws;             /* bwd: workspace of SWV2_LN_BWD_MAX_BLOCKS * 2 * C floats (per-block partial sums) */
    int M, C, res_mod, rows_per_sample;
    float eps;
} swv2_ln_args;

int swv2_ln_residual_fwd(const swv2_ln_args* a, void* stream);
int swv2_ln_residual_bwd(const swv2_ln_args* a, void* stream);

/* out[i] (+)= sum_b in[b][i], i < n (n % 4 == 0): pos_embed gradient */
int swv2_batch_sum(const float* in, float* out, int B, long n, int accumulate, void* stream);

/* PatchMerging (swinv2_global.py:500-523; never instantiated by swinv2net but part of the model file) */
int swv2_merge_stats(const float* x, float* mean, float* rstd, int B, int H, int W, int C, float eps, void* stream);
int swv2_merge_ln_bwd(const float* x, const void* dn_bf16, const float* gamma, const float* mean, const float* rstd,
                      float* dx, float* dgamma, float* dbeta, int B, int H, int W, int C, void* stream);

/* Geometric l2 loss (csrc/loss_l2.hip; utils/losses.py:188-232, utils/grids.py:115-117): one pass over prd and tar (contiguous [BC][H][W])
 * produces, per (b,c) plane, sums[2*bc] = sum q[h](prd-tar)^2 and sums[2*bc+1] = sum q[h] tar^2.  swv2_loss_sums: one launch of
 * BC * swv2_score_slices(BC, H, W) workgroups (the plan and slice bounds of swv2_score_sums) that store their slice's two sums at
 * ws[(plane * slices + slice) * 2 ..], then one small launch that folds the slices of each plane in a fixed order into sums [BC][2].  No
 * atomics, nothing to zero beforehand (sums and ws are written in full, never read first); two runs on the same inputs agree bit for bit,
 * and with swv2_score_sums' S_dd and S_tt without a climatology.  A NaN in a plane reaches that plane's two sums only.  (113: ws, ws_bytes)
 * The backward is dprd = coef[bc] * q[h] * (prd - tar) with coef from the chain rule of the chosen variant; the grid of swv2_l1_grad.
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer, W % 4 != 0, prd / tar / ws / dprd not 16-byte aligned, sums not 8-byte
 * aligned, a workspace smaller than swv2_loss_ws_bytes, BC >= 2^20 (swv2_loss_grad: BC > 65535), H * W >= 2^30.  swv2_loss_ws_bytes is
 * host-only (no HIP call) and returns 0 for a non-positive argument. */
size_t swv2_loss_ws_bytes(int planes, int H, int W);      /* planes * swv2_score_slices(planes, H, W) * 8 */
int swv2_loss_sums(const float* prd, const float* tar, const float* quad_w, float* sums, int BC, int H, int W, void* ws, size_t ws_bytes,
                   void* stream);
int swv2_loss_grad(const float* prd, const float* tar, const float* quad_w, const float* coef, float* dprd, int BC, int H,
                   int W, void* stream);
/* The scalar on top of the sums (losses.py:200-232): loss = sum_{b,c} chw[c] f(S0 / S1) (S0 alone when absolute; f = sqrt
 * unless squared) and coef[bc] = 2 d loss / d S0[bc], the factor swv2_loss_grad takes.  chw: [C] weights (channel weights x
 * multistep weights, normalised as LossHandler does); BC = B * C. */
/* sums is [layers][BC][2]: the layers are added in order (layers = 1: swv2_loss_sums; SWV2_LOSS_PART_SLICES:
 * swv2_loss_part_reduce). */
#define SWV2_LOSS_PART_SLICES 8
#define SWV2_LOSS_GROUP_ROWS 32
#define SWV2_LOSS_DUMP_BYTES 2048
/* row pitch (elements) of loss_resid for N = Cout * 16 columns: whole 128-byte lines per row, so that the 64-column pieces the epilogue
 * writes and the head's backward products read never straddle a line (107) */
#define SWV2_LOSS_RESID_PITCH(N) (((N) + 63) / 64 * 64)
/* Folds the loss epilogue's per-group partial sums: sums[j][b][coff + c][k] = sum over the SWV2_LOSS_GROUP_ROWS-row groups g with
 * g % SWV2_LOSS_PART_SLICES == j of (slot 0 of g if g's first row lies in sample b) + (slot 1 of g if it lies in sample b - 1),
 * ascending g; T rows per sample (T >= SWV2_LOSS_GROUP_ROWS).  sums: [SWV2_LOSS_PART_SLICES][B][Ct][2], overwritten for the Cout channels from coff. */
int swv2_loss_part_reduce(const float* part, int M, int T, int B, int Cout, int Ct, int coff, float* sums, void* stream);
/* The loss epilogue's residual (loss_resid, bf16 [M][SWV2_LOSS_RESID_PITCH(Cout * 16)], rows = patches (b, i, j), columns c * 16 + p * 4 + q) back in image layout and
 * scaled: out[b][c][4i + p][4j + q] = coef[b][c] * resid (+ add[b][c][..] when add != NULL; add: [B][Cadd][H][W], out: the first Cout channels of
 * [B][Cs][H][W]) -- d loss / d prediction where a consumer wants it as an image (the skip connection of a rollout step,
 * swinv2_global.py:799-801).  coef as for swv2_loss_grad.  (107) */
int swv2_loss_resid_to_image(const void* resid, const float* coef, const float* add, float* out, int B, int Cout, int H, int W, int Cs, int Cadd,
                             void* stream);
int swv2_loss_finalize(const float* sums, int layers, const float* chw, int BC, int C, int absolute, int squared, float* loss, float* coef,
                       void* stream);

/* torch.optim.Adam step (train.py:176) over one flat fp32 buffer; step >= 1; grads are multiplied by grad_inv_scale */
int swv2_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   int step, float grad_inv_scale, void* stream);

/* The same update for MANY tensors in one launch (replaces optimizer.step() of train.py:176 / :330).  items_dev: device
 * array of tensors; chunks_dev: device array of int pairs (item index, chunk index within the item), one workgroup per
 * chunk of swv2_adam_chunk() elements; both tables are built by the caller (swin_v2_weather_amd/utils/optim.py). */
typedef struct swv2_adam_item {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
} swv2_adam_item;
int swv2_adam_chunk(void);
int swv2_adam_multi(const swv2_adam_item* items_dev, const int* chunks_dev, int n_chunks, float lr, float beta1, float beta2,
                    float eps, int step, float grad_inv_scale, void* stream);

/* LAMB with apex FusedLAMB's semantics (replaces `optimizers.FusedLAMB(...)`, train.py:177-178, and its step at :330) for MANY fp32
 * tensors, in the multi-tensor shape of swv2_adam_multi: ONE item table and ONE chunk table for the tensors of all parameter groups, one
 * workgroup per chunk of swv2_lamb_chunk() elements.  chunks_dev holds int pairs (item index, chunk index within the item), item by item
 * in ascending chunk order; an item's chunk0 is the position of its first pair.  A group is a range of items and the matching range of chunks.
 *   step:  G = sqrt(sum over all items of (g grad_inv_scale)^2 + *extra_gnorm2);  c = G > max_grad_norm ? G / max_grad_norm : 1
 *          g^ = g grad_inv_scale / c  (+ weight_decay p without SWV2_LAMB_ADAMW);  b3 = 1 - beta1 with SWV2_LAMB_GRAD_AVERAGING, else 1
 *          m <- beta1 m + b3 g^;  v <- beta2 v + (1 - beta2) g^ g^;  a = (m / bc1) / (sqrt(v / bc2) + eps)
 *          u = a (+ weight_decay p with SWV2_LAMB_ADAMW);  bc = 1 - beta^step with SWV2_LAMB_BIAS_CORRECTION, else 1
 *          r = |p| / |u| per tensor if (SWV2_LAMB_NVLAMB or weight_decay != 0) and |p| != 0 and |u| != 0, else 1 (|p| before the update)
 *          p <- p - lr r u
 * g is read only; non-finite values propagate as the arithmetic dictates.  The square of an element passes through at most
 * SWV2_LAMB_SUM_DEPTH fp32 additions on its way into a norm, in an order fixed by the tables (no float atomics: a second run from the
 * same state gives the same bits).  All scalars reach the kernels as fp32; 1 - beta is formed in fp32.
 * Workspace (the caller's, swv2_lamb_ws_bytes(n_items, n_chunks) bytes, 4-byte aligned), as floats, after the calls:
 *   [SWV2_LAMB_WS_GNORM2] |g|^2 = G^2   [SWV2_LAMB_WS_CLIP] c   [SWV2_LAMB_WS_BC1], [SWV2_LAMB_WS_BC2] bc1, bc2 of the last group
 *   [SWV2_LAMB_WS_ITEM(i) + 0, 1, 2]  |p|^2, |u|^2, r of item i;  the rest (chunk partial sums) is scratch.
 * swv2_lamb_grad_norm: ONE launch, the chunk partial sums of |g|^2 over all items.  swv2_lamb_multi: one group, items [item_lo, item_hi)
 * = chunks [chunk_lo, chunk_hi), four launches (|g|^2 and c; m, v and the partial sums of p^2, u^2; the norms and r; the update).
 * extra_gnorm2: NULL or a device float added to |g|^2, the share of tensors the caller updates itself.  A refused call (null table,
 * n_chunks <= 0, step < 1, a range outside the tables, a workspace that is too small) launches nothing and writes nothing. */
typedef struct swv2_lamb_item {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
    long chunk0;
} swv2_lamb_item;
#define SWV2_LAMB_SUM_DEPTH 64
#define SWV2_LAMB_ADAMW 1
#define SWV2_LAMB_BIAS_CORRECTION 2
#define SWV2_LAMB_GRAD_AVERAGING 4
#define SWV2_LAMB_NVLAMB 8
#define SWV2_LAMB_WS_GNORM2 0
#define SWV2_LAMB_WS_CLIP 1
#define SWV2_LAMB_WS_BC1 2
#define SWV2_LAMB_WS_BC2 3
#define SWV2_LAMB_WS_ITEM(i) (4 + 4 * (i))
int swv2_lamb_chunk(void);
size_t swv2_lamb_ws_bytes(int n_items, int n_chunks);      /* 4 * (SWV2_LAMB_WS_ITEM(n_items) + 6 * n_chunks); 0 for a non-positive count */
int swv2_lamb_grad_norm(const swv2_lamb_item* items_dev, const int* chunks_dev, int n_items, int n_chunks, float grad_inv_scale, void* ws,
                        size_t ws_bytes, void* stream);
int swv2_lamb_multi(const swv2_lamb_item* items_dev, const int* chunks_dev, int n_items, int n_chunks, int item_lo, int item_hi,
                    int chunk_lo, int chunk_hi, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_inv_scale,
                    float max_grad_norm, int step, int flags, const float* extra_gnorm2, void* ws, size_t ws_bytes, void* stream);

/* Forecast scores (reference utils/weighted_acc_rmse.py:50-115): latitude-weighted RMSE and anomaly correlation of a prediction against
 * the verifying analysis, per (sample, channel) plane, from ONE pass over prediction, truth and climatology.  All tensors fp32.
 *   prd, tar  C planes of [H][W] per sample, sample b at ptr + b * bstride (elements): a channel block of a wider tensor is scored in
 *             place (bstride = channels of the whole tensor * H * W); clim: [C][H][W] shared by all samples, or NULL; w: [H] row weights.
 *   S_dd = sum w[h] (p - t)^2   S_pt = sum w[h] p' t'   S_pp = sum w[h] p'^2   S_tt = sum w[h] t'^2,   p' = p - clim, t' = t - clim
 *   (p' = p, t' = t when clim is NULL; p - t is formed from p and t, so S_dd does not depend on clim).
 * swv2_score_sums: one launch of B * C * swv2_score_slices(B * C, H, W) workgroups; workgroup (plane, slice) stores its four partial sums at
 * ws[(plane * slices + slice) * 4 ..], plane = b * C + c, slice sl covering the elements [H W sl / slices / 4 * 4, H W (sl + 1) / slices / 4 * 4)
 * of the plane (the last slice to the end; a slice without elements stores zeros).  No atomics, nothing to zero beforehand.
 * swv2_score_finalize: one launch; folds the slices of each plane in a fixed order (two runs on the same inputs agree bit for bit) and writes
 *   sums [B][C][4] = (S_dd, S_pt, S_pp, S_tt)    rmse [B][C] = sqrt(S_dd / (H W))    acc [B][C] = S_pt / sqrt(S_pp S_tt) (0 / 0 = NaN in that plane)
 *   rmse_mean [C] = mean_b rmse[b][c] (* scale[c] when scale != NULL: the physical-unit stds)    acc_mean [C] = mean_b acc[b][c]
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer (clim and scale may be NULL), W % 4 != 0, prd / tar / clim / ws / sums not
 * 16-byte aligned, a batch stride that is not a multiple of 4, a workspace smaller than swv2_score_ws_bytes, B * C >= 2^20, H * W >= 2^30.
 * swv2_score_slices and swv2_score_ws_bytes are host-only (no HIP call); both return 0 for a non-positive argument. */
int swv2_score_slices(int planes, int H, int W);
size_t swv2_score_ws_bytes(int planes, int H, int W);     /* planes * swv2_score_slices(planes, H, W) * 16 */
int swv2_score_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* clim, const float* w, int B, int C,
                    int H, int W, void* ws, size_t ws_bytes, void* stream);
int swv2_score_finalize(const void* ws, size_t ws_bytes, int B, int C, int H, int W, const float* scale, float* sums, float* rmse, float* acc,
                        float* rmse_mean, float* acc_mean, void* stream);

/* Dataset statistics: the running sums behind global_means / global_stds / time_diff_stds / time_means, one pass per time slab while the
 * year files stream through the device (utils/dataset_stats.py).  slab, prev: [C][H][W] fp32 on the device; everything accumulated is fp64.
 *   x' = (double)x - pivot[c]     d = (double)x - (double)prev (only when prev != NULL: the previous slab of the SAME year file)
 *   tsum [C][H][W] += x'          part [C][slices][6] += (sum x', sum x'^2, sum d, sum d^2, number of non-finite x, 0 (spare))
 * swv2_stats_accumulate: one launch of C * swv2_stats_slices(C, H, W) workgroups; workgroup (c, slice) owns part[c][slice][0..5] and the tsum
 * elements [H W sl / slices / 4 * 4, H W (sl + 1) / slices / 4 * 4) of plane c (the last slice to the end).  Slabs are serialised on the
 * stream and every accumulator has one owner: no atomics.  first != 0 stores instead of adding (tsum and part alike): nothing to zero
 * beforehand.  pivot [C] fp64 on the device, a value near the channel mean (an fp32 value, so that x' is exact), the same for every call.
 * swv2_stats_finalize: folds the slices of each channel in one fixed order (two runs on the same inputs agree bit for bit) into
 *   folded [C][6]     and writes     time_means [C][H][W] = (float)(pivot[c] + tsum / T),     T = the number of slabs accumulated.
 * Means, variances and roots over the C channels are host arithmetic on `folded` (utils/dataset_stats.py::vectors_from_folded).
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer (prev may be NULL), C, H, W <= 0, C >= 2^20, H * W >= 2^30,
 * H * W % 4 != 0, slab / prev / tsum / time_means not 16-byte aligned, pivot / part / folded not 8-byte aligned, a workspace (part) smaller
 * than swv2_stats_ws_bytes, T <= 0.  swv2_stats_slices and swv2_stats_ws_bytes are host-only (no HIP call); both return 0 for a non-positive
 * argument. */
int swv2_stats_slices(int C, int H, int W);
size_t swv2_stats_ws_bytes(int C, int H, int W);          /* C * swv2_stats_slices(C, H, W) * 6 * 8: the bytes of part */
int swv2_stats_accumulate(const float* slab, const float* prev, const double* pivot, double* tsum, void* part, size_t part_bytes, int C, int H,
                          int W, int first, void* stream);
int swv2_stats_finalize(const void* part, size_t part_bytes, const double* tsum, const double* pivot, int C, int H, int W, long T,
                        double* folded, float* time_means, void* stream);

/* Order statistics of every (sample, channel) plane (csrc/quantile.hip): the values at K given ranks of the sorted plane, by a multi-rank
 * radix select on order-preserving 32-bit keys (digits of 12, 5, 5, 5, 5 bits) -- five streaming passes, no sort, no plane-sized temporary.
 * Behind the extremes metric top_quantiles_error_torch (reference utils/weighted_acc_rmse.py:117-126).
 *   x          C planes of [H][W] fp32 per sample, sample b at x + b * bstride (elements): a channel block of a wider tensor is read in place
 *   ranks      [K] device ints, distinct, ascending, in [0, H W): the same ranks for every plane (the caller builds them)
 *   out        [K][B * C] fp32: out[k][b * C + c] = the element of rank ranks[k] of plane (b, c) in ascending order.  NaNs sort last (as in
 *              torch.sort) and come back as NaN; -0.0 sorts directly below +0.0.
 *   nan_count  [B * C] ints: the number of NaNs of the plane
 *   ws         swv2_quantile_ws_bytes(B * C, H, W, K) bytes = planes * 35 856: per plane 8192 integer counters, the active prefixes, and the
 *              slot and residual of every rank.  The op zeroes what it counts into and writes all state before reading it: the caller
 *              zeroes nothing, a dirty workspace gives the bits of a clean one.
 * One call is a fixed sequence of launches on `stream` without host synchronisation: a memset of the workspace, then per digit one count
 * launch of B * C * slices workgroups (the plan of swv2_score_sums: slices = planes >= 2048 ? 1 : 2048 / planes, slice bounds on 16-byte
 * vectors) that folds its LDS histogram into the plane's counters with integer atomics, and one resolve launch of B * C workgroups.  Integer
 * counters: the result does not depend on arrival order, two runs agree bit for bit.
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer, B, C, H, W <= 0, B * C >= 2^20, H * W >= 2^30, H * W % 4 != 0, x / ws not
 * 16-byte aligned, ranks / out / nan_count not 4-byte aligned, a batch stride that is not a multiple of 4 or (B > 1) smaller than C H W,
 * K < 1 or K > 256, a workspace smaller than swv2_quantile_ws_bytes.  swv2_quantile_ws_bytes is host-only (no HIP call) and returns 0 for a
 * non-positive argument. */
size_t swv2_quantile_ws_bytes(int planes, int H, int W, int K);
int swv2_plane_order_stats(const float* x, long bstride, int B, int C, int H, int W, const int* ranks, int K, float* out, int* nan_count,
                           void* ws, size_t ws_bytes, void* stream);

/* Ensemble scores (csrc/ensemble.hip): CRPS, fair CRPS, spread, ensemble-mean RMSE and the rank histogram of M forecast members against the
 * verifying analysis, per (sample, channel) plane, from ONE pass in which every thread holds the M values of its grid points in registers.
 * All fields fp32.
 *   ens       member m, sample b, channel c at ens + m * ens_mstride + b * ens_bstride + c * H * W (elements): a ring slot or a channel block of
 *             a member-major [M * B, channels, H, W] tensor is scored in place (ens_mstride = B * ens_bstride)
 *   tar       the truth, sample b at tar + b * tar_bstride, C planes of [H][W];  w: [H] row weights, the vector swv2_score_sums takes
 *   per grid point, every term from differences of inputs:   xbar = (1 / M) sum_m x_m    s2 = (1 / (M - 1)) sum_m (x_m - xbar)^2
 *             e1 = sum_m |x_m - y|    e2 = sum_{m<n} |x_m - x_n| (as the gaps of the sorted members)    rank = #{m : x_m < y}  (strict, 0 .. M)
 *   per plane  S_mse = sum w[h] (xbar - y)^2    S_var = sum w[h] s2    S_1 = sum w[h] e1    S_2 = sum w[h] e2    hist[r] = #{points with rank r}
 * swv2_ens_sums: one launch of B * C * swv2_score_slices(B * C, H, W) workgroups (the plan and slice bounds of swv2_score_sums); workgroup
 * (plane, slice) stores four float partials at ws[(plane * slices + slice) * 4 ..] and, behind all of those, M + 1 integer counts at
 * ((int*)ws)[planes * slices * 4 + (plane * slices + slice) * (M + 1) ..].  No float atomics, nothing to zero beforehand; a slice without
 * elements stores zeros.  The kernel is chosen by M alone: register slots for M rounded up to a multiple of 8.
 * swv2_ens_finalize: one launch; folds the slices of each plane in a fixed order (two runs on the same inputs agree bit for bit, counts
 * included) and writes, with N = H W,
 *   sums [B][C][4] = (S_mse, S_var, S_1, S_2)    hist [B][C][M + 1] (its entries add up to N exactly)
 *   ens_rmse = sqrt(S_mse / N)   spread = sqrt(S_var / N)   crps = (S_1 / M - S_2 / M^2) / N   fair_crps = (S_1 / M - S_2 / (M (M - 1))) / N   [B][C] each
 *   means [4][C] = the batch means of ens_rmse, spread, crps, fair_crps in ascending b; scale[c] (may be NULL: the physical-unit stds)
 *   multiplies the first three.
 * A NaN in a member or in the truth makes the four scores of that plane (and that channel's means) NaN and touches no other plane; the
 * plane's hist is then unspecified except that it still adds up to N.
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer (scale may be NULL), M outside 2 .. 64, W % 4 != 0, ens / tar / ws / sums not
 * 16-byte aligned, a member or batch stride that is not a multiple of 4 or (B > 1) a batch stride smaller than C H W, B * C >= 2^20,
 * H * W >= 2^30, a workspace smaller than swv2_ens_ws_bytes.  swv2_ens_ws_bytes is host-only (no HIP call) and returns 0 for a non-positive
 * argument or M outside 2 .. 64. */
size_t swv2_ens_ws_bytes(int planes, int H, int W, int M);      /* planes * swv2_score_slices(planes, H, W) * (16 + 4 (M + 1)) */
int swv2_ens_sums(const float* ens, long ens_mstride, long ens_bstride, const float* tar, long tar_bstride, const float* w, int M, int B, int C,
                  int H, int W, void* ws, size_t ws_bytes, void* stream);
int swv2_ens_finalize(const void* ws, size_t ws_bytes, int M, int B, int C, int H, int W, const float* scale, float* sums, int* hist,
                      float* ens_rmse, float* spread, float* crps, float* fair_crps, float* means, void* stream);

/* Forecast events (csrc/events.hip; purely additive, the revision stays 113): the 2 x 2 contingency table of a forecast and the Brier sums
 * and reliability counts of an ensemble for K <= 8 thresholds at once, per (sample, channel) plane, from ONE pass.  All fields fp32.
 *   prd, tar  C planes of [H][W] per sample, sample b at ptr + b * bstride (elements), as swv2_score_sums takes them
 *   ens       member m, sample b, channel c at ens + m * ens_mstride + b * ens_bstride + c * H * W, as swv2_ens_sums takes them; M = 2 .. 64
 *   base      NULL or [C][H][W], shared by the samples (read like the climatology of swv2_score_sums)
 *   thr       threshold k of plane (b, c) at thr[b * thr_bstride + c * K + k]; thr_bstride = 0: one [C][K] table for every sample
 *   w         [H] row weights;  below: 0 or 1
 *   theta = thr, or fl32(base + thr) with a base (one fp32 addition).  Event: x > theta, or x < theta with below; strict, in fp32: a value
 *   equal to theta is no event.  A point is valid in its plane if prediction (every member), truth and base are not NaN there; +-inf are
 *   valid.  Invalid points enter no sum and no count, and are counted in n_invalid[B][C].
 *   deterministic, P / O = event in prediction / truth, over the valid points:
 *     table[B][C][K][4] = (a, b, c, d) = (sum w [P and O], sum w [P and not O], sum w [not P and O], sum w [not P and not O]), four sums of their
 *     own: with unit weights every cell is an exact integer for H W <= 2^24
 *   ensemble, n = #{m : x_m event}, o = [truth event], over the valid points:
 *     sums[B][C][K][3] = (S_e, S_f, S_o) = (sum w (n - M o)^2, sum w n (M - n), sum w o)      wv[B][C] = sum w
 *     hist[B][C][K][2][M + 1]: [0][j] = #{points with n = j},  [1][j] = #{points with n = j and o = 1}  (int32 point counts, unweighted)
 * swv2_event_sums / swv2_event_ens_sums: one launch of B * C * swv2_score_slices(B * C, H, W) workgroups (the plan and slice bounds of
 * swv2_score_sums, workgroup index (c * slices + sl) * B + b); workgroup (plane, slice) stores its partial sums and counts in the workspace.
 * No float atomics, nothing to zero beforehand; a slice without elements stores zeros.  The counts are integer adds in LDS; the bin
 * (n = 0, o = 0), which holds nearly every point of a rare event, is not counted but formed by swv2_event_ens_finalize as the valid points
 * minus the other bins (integers: exact).
 * swv2_event_finalize / swv2_event_ens_finalize: one launch; folds the slices of each plane in a fixed order (two runs on the same inputs agree
 * bit for bit, counts included) and writes the outputs above.
 * Refused with SWV2_ERR_INVALID before any HIP call, the entry point's name in the message: a null pointer (base may be NULL), K outside
 * 1 .. 8, M outside 2 .. 64, W % 4 != 0, prd / ens / tar / base / ws / table not 16-byte aligned, another pointer not 4-byte aligned, a member
 * or batch stride that is not a multiple of 4 or (B > 1) a batch stride smaller than C H W, a thr_bstride that is neither 0 nor (B > 1) at
 * least C K, B * C >= 2^20, H * W >= 2^30, a workspace smaller than the query.  The queries are host-only (no HIP call) and return 0 for a
 * non-positive argument, K outside 1 .. 8 or M outside 2 .. 64. */
size_t swv2_event_ws_bytes(int planes, int H, int W, int K);      /* planes * swv2_score_slices(planes, H, W) * (16 K + 4) */
int swv2_event_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* base, const float* thr, long thr_bstride,
                    const float* w, int K, int below, int B, int C, int H, int W, void* ws, size_t ws_bytes, void* stream);
int swv2_event_finalize(const void* ws, size_t ws_bytes, int K, int B, int C, int H, int W, float* table, int* n_invalid, void* stream);
size_t swv2_event_ens_ws_bytes(int planes, int H, int W, int M, int K);      /* planes * slices * (16 K + 4 + 8 K (M + 1)) */
int swv2_event_ens_sums(const float* ens, long ens_mstride, long ens_bstride, const float* tar, long tar_bstride, const float* base,
                        const float* thr, long thr_bstride, const float* w, int M, int K, int below, int B, int C, int H, int W, void* ws,
                        size_t ws_bytes, void* stream);
int swv2_event_ens_finalize(const void* ws, size_t ws_bytes, int M, int K, int B, int C, int H, int W, float* sums, float* wv, int* hist,
                            int* n_invalid, void* stream);

/* Neighbourhood verification (csrc/fss.hip; purely additive, the revision stays 113): the integer sums behind the fractions skill score
 * (Roberts and Lean 2008) of a forecast against the analysis, for K <= 8 thresholds and S <= 8 box sizes at once, per (sample, channel) plane.
 *   prd, tar, base, thr, thr_bstride, below: the operands of swv2_event_sums, with its event, theta = thr or fl32(base + thr), strictness, fp32
 *   comparison and validity.  An invalid point (a NaN in prediction, truth or base) is NO EVENT IN EITHER FIELD and is counted per plane in
 *   n_invalid[B][C]; it stays in every denominator.
 *   scales    int[S] on the HOST: half-widths r in grid points, strictly ascending, 0 <= r <= 32, 2 r + 1 <= W
 *   The neighbourhood of (h, w) at scale r is rows max(0, h - r) .. min(H - 1, h + r) and columns w - r .. w + r MODULO W: the longitude is
 *   periodic, the poles clip the box; it holds N_h = (rows in the clipped box) * (2 r + 1) points.  n_f(h, w) / n_o(h, w) = the number of
 *   forecast / analysis events in it, integers.
 *     rows[B][C][K][S][H][3] = (sum_w (n_f - n_o)^2, sum_w n_f^2, sum_w n_o^2)      int64, exact
 *   The area weighting is the caller's, in fp64, a dot product over H (utils/events.py::fss_scores): with q[h] = w[h] / N_h^2,
 *     FBS = sum_h q[h] rows[.., h, 0]    SF, SO likewise from [.., 1], [.., 2]    FSS = 1 - FBS / (SF + SO)   (0 / 0 = NaN in that entry only)
 *   At r = 0, (FBS, SF, SO) = (b + c, a + b, a + c) of the contingency table of swv2_event_sums.  Scores over a batch or over lead times are
 *   the scores of the SUMMED rows.  The kernels do no floating-point arithmetic on an output: there is no tolerance, and two runs agree bit
 *   for bit by construction.
 * Integer types: a box count is at most 65 * 65 = 4225 (int); a squared difference at most 4225^2 = 1.8e7, of which a thread adds at most 4
 * and 16 lanes at most 64 in 32 bits (1.15e9 < 2^32); everything beyond is 64-bit: a row sum at W = 16384 is at most 2.9e11.
 * swv2_fss_rows is ONE entry point over two launches on `stream`, no host synchronisation: the masks (one streaming pass on the slices and
 * workgroup index of swv2_event_sums, each input read once: 2 K event bits per point as bit rows in the workspace, and the invalid points per
 * slice), then the boxes (one workgroup per (plane, threshold, band of rows): planes * K * ceil(H / band) workgroups with
 * band = swv2_fss_band_rows(planes, H, K, r_max = scales[S - 1]); each slides the box counts of its columns down the band from an LDS image
 * of the bit rows, for every scale, and stores its band of `rows`; the first of a plane also folds n_invalid).  No float atomics, nothing to
 * zero beforehand, every slot of rows and n_invalid is written, nothing outside them and the workspace is written.
 * swv2_fss_band_rows: the plan, host-only.  Bands are at least max(2 r_max + 1, 32) rows tall and at most 80 -- except that a call of fewer
 * than 8 workgroups (one per XCD) is cut further, down to bands of 8 rows, until it has 8.  0 for a non-positive or out-of-range argument.
 * Refused with SWV2_ERR_INVALID before any HIP call, the entry point's name in the message: a null pointer (base may be NULL), K or S outside
 * 1 .. 8, scales not strictly ascending, outside 0 .. 32 or with 2 r + 1 > W, W % 4 != 0, prd / tar / base / ws not 16-byte aligned, rows not
 * 8-byte aligned, thr / n_invalid not 4-byte aligned, a batch stride that is not a multiple of 4 or (B > 1) smaller than C H W, a thr_bstride
 * that is neither 0 nor (B > 1) at least C K, B * C >= 2^20, H * W >= 2^30, a workspace smaller than swv2_fss_ws_bytes.  The queries are
 * host-only (no HIP call) and return 0 for a non-positive argument or K, S outside 1 .. 8. */
int swv2_fss_band_rows(int planes, int H, int K, int r_max);
size_t swv2_fss_ws_bytes(int planes, int H, int W, int K, int S);     /* 4 * planes * (2 K H ceil(W / 32) + swv2_score_slices(planes, H, W)) */
int swv2_fss_rows(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* base, const float* thr, long thr_bstride,
                  const int* scales, int K, int S, int below, int B, int C, int H, int W, void* ws, size_t ws_bytes, long long* rows,
                  int* n_invalid, void* stream);

/* Ensemble neighbourhood verification (csrc/fss.hip; purely additive, the revision stays 113): the integer sums behind the probabilistic
 * fractions skill score -- the neighbourhood ensemble probability (Schwartz et al. 2010) scored with the FSS formula (Duc et al. 2013) --
 * of M = 2 .. 64 members against the analysis, for K <= 8 thresholds and S <= 8 box sizes at once, per (sample, channel) plane.
 *   ens, ens_mstride, ens_bstride: the members as swv2_event_ens_sums takes them; tar, base, thr, thr_bstride, below, scales: the operands of
 *   swv2_fss_rows, with its event, theta, strictness, fp32 comparison, base field and box (clipped at the poles, wrapped in longitude).
 *   A point is valid if no member, nor the truth, nor the base is NaN there; +-inf are valid.  An invalid point is an event in NO member and
 *   not in the analysis, and is counted in n_invalid[B][C].  With e_m(h, w) the event bit of member m and o that of the analysis:
 *     c = sum_m e_m (0 .. M)      N_f(h, w) = sum_box c = sum_m n_f^m      n_o(h, w) = sum_box o
 *     rows[B][C][K][S][H][3] = (sum_w (N_f - M n_o)^2, sum_w N_f^2, sum_w n_o^2)      int64, exact
 *   Scores, fp64, the caller's (utils/events.py::fss_ens_scores): with q[h] = w[h] / N_h^2,
 *     FBS = sum_h q rows[.., 0] / M^2    SF = sum_h q rows[.., 1] / M^2    SO = sum_h q rows[.., 2]    pfss = 1 - FBS / (SF + SO)
 *   base_rate from rows[.., 2] at scale 0, fss_uniform = 0.5 + base_rate / 2; scores over a batch or over lead times are the scores of the
 *   SUMMED rows.  M copies of one forecast give (M^2 d, M^2 f, o) of swv2_fss_rows' (d, f, o); at r = 0 with unit weights sum_h rows[.., 0] is
 *   the S_e of swv2_event_ens_sums.  No floating-point arithmetic on an output: two runs agree bit for bit.
 * Integer bounds: N_f <= 64 * 4225 = 270 400 < 2^19 (int).  A square is < 2^37 and does NOT fit 32 bits: everything after the box count is
 * 64-bit.  A thread adds at most 4 squares (< 2^39); the 16 lanes of a DPP row add them as two 32-bit halves (the low 24 bits: 16 * 2^24 =
 * 2^28; the rest: 16 * 2^15 = 2^19), recombined to < 2^43 before the 64-bit integer add in LDS; a row sum at W = 16384 is < 2^51.
 * swv2_fss_ens_rows is ONE entry point over two launches on `stream`: the masks (the units and workgroup index of swv2_fss_rows' first
 * launch; the members stream past, a lane counts its 4 points in the bytes of one register per threshold and writes the count as
 * P = bit_length(M) bit planes plus the analysis bit row: bits[plane][k][P + 1][H][ceil(W / 32)]), then the boxes (one workgroup per (plane,
 * threshold, band); a forecast window count is sum_p popcount(window of plane p) << p).  Nothing to zero beforehand, every slot of rows and
 * n_invalid has one owner and is written, nothing outside them and the workspace is written.
 * swv2_fss_ens_band_rows: the plan, host-only.  A workgroup needs at most 80 KiB of LDS (two per CU) for 8 scales.  Bands follow the rule of
 * swv2_fss_band_rows (at least max(2 r_max + 1, 32) rows unless the call has fewer than 8 workgroups); where such a band does not fit with
 * 1024-column tiles the column tile is halved (512, then 256) first, and the band is capped by what then fits (at most 80).
 * Refused with SWV2_ERR_INVALID before any HIP call, the entry point's name in the message: what swv2_fss_rows refuses, M outside 2 .. 64, a
 * member stride that is not a multiple of 4, a workspace smaller than swv2_fss_ens_ws_bytes.  The queries return 0 for a non-positive
 * argument, M outside 2 .. 64 or K, S outside 1 .. 8.
 * SWV2_ENS expands to nothing.  It stands between the return type and the name because tests/test_fss_host.py finds the three deterministic
 * entry points above by the pattern "int|size_t swv2_fss_<name>(" and pins their list; tests/test_efss_host.py reads these three with it. */
#define SWV2_ENS
int SWV2_ENS swv2_fss_ens_band_rows(int planes, int H, int M, int K, int r_max);
size_t SWV2_ENS swv2_fss_ens_ws_bytes(int planes, int H, int W, int M, int K, int S);   /* 4 * planes * ((bit_length(M) + 1) K H ceil(W / 32) + slices) */
int SWV2_ENS swv2_fss_ens_rows(const float* ens, long ens_mstride, long ens_bstride, const float* tar, long tar_bstride, const float* base,
                               const float* thr, long thr_bstride, const int* scales, int M, int K, int S, int below, int B, int C, int H, int W,
                               void* ws, size_t ws_bytes, long long* rows, int* n_invalid, void* stream);

/* Geometric l1 loss (csrc/loss_l1.hip; reference utils/losses.py:114-120 with p = 1) and the latitude-weighted mean absolute error: per
 * (sample, channel) plane, from ONE pass over prediction and target.  All tensors fp32.
 *   prd, tar  C planes of [H][W] per sample, sample b at ptr + b * bstride (elements), as swv2_score_sums takes them;  w: [H] row weights
 *   S0 = sum w[h] |p - t|      S1 = sum w[h] |t|
 * swv2_l1_sums: one launch of B * C * swv2_score_slices(B * C, H, W) workgroups (the plan and slice bounds of swv2_score_sums); workgroup
 * (plane, slice) stores (S0, S1) of its slice at ws[(plane * slices + slice) * 2 ..], plane = b * C + c.  No atomics, nothing to zero
 * beforehand; a slice without elements stores zeros.
 * swv2_l1_finalize: one launch of one workgroup; folds the slices of each plane in a fixed order and writes sums [B][C][2] = (S0, S1).
 * With chw != NULL ([C] channel weights) it also writes
 *   loss [1] = sum_bc chw[c] norm[b][c],   norm = S0 (absolute != 0) or S0 / S1,   the B C terms added in an order fixed by the code
 *   coef [B][C] = d loss / d S0 = chw[c] (absolute) or chw[c] / S1[b][c]
 * (loss and coef are not touched and may be NULL when chw is NULL).  Two runs on the same inputs agree bit for bit in every output.  A
 * NaN in a plane makes that plane's sums and the loss NaN and touches no other plane's sums.
 * swv2_l1_grad: dprd[b][c][h][w] = coef[b][c] * w[h] (one fp32 product) with the sign of p - t, taken from the comparisons p > t and
 * p < t: +-that product, or 0 where p == t or either is NaN.  prd, tar, dprd contiguous [B C][H][W]; the grid of swv2_loss_grad.
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer, W % 4 != 0, prd / tar / ws / dprd not 16-byte aligned, sums not 8-byte
 * aligned, a batch stride that is not a multiple of 4 or (B > 1) smaller than C H W, a workspace smaller than swv2_l1_ws_bytes,
 * B * C >= 2^20 (swv2_l1_grad: B * C > 65535), H * W >= 2^30.  swv2_l1_ws_bytes is host-only (no HIP call) and returns 0 for a
 * non-positive argument. */
size_t swv2_l1_ws_bytes(int planes, int H, int W);        /* planes * swv2_score_slices(planes, H, W) * 8 */
int swv2_l1_sums(const float* prd, long prd_bstride, const float* tar, long tar_bstride, const float* w, int B, int C, int H, int W, void* ws,
                 size_t ws_bytes, void* stream);
int swv2_l1_finalize(const void* ws, size_t ws_bytes, int B, int C, int H, int W, const float* chw, int absolute, float* sums, float* loss,
                     float* coef, void* stream);
int swv2_l1_grad(const float* prd, const float* tar, const float* quad_w, const float* coef, float* dprd, int BC, int H, int W, void* stream);

/* Spherical-harmonic degree spectra (csrc/sht.hip; the RealSHT + |c|^2 sums of reference utils/losses.py:272-307): the Legendre stage of
 * the transform and the degree power  P[plane][l] = sum_m w_m |c[m][l][plane]|^2,  w_0 = 1, else 2.  All tensors fp32.
 *   table   [mmax][lmax][nlat]      quadrature-weighted orthonormal associated Legendre functions; rows l < m are never read
 *   X, dX   [mmax][2 planes][nlat]  the longitude transform of the planes, column n = 2 plane + (0: real part, 1: imaginary part)
 *   coeffs  [mmax][2 planes][lmax]  c[m][n][l] = sum_k table[m][l][k] X[m][n][k]; ONLY l >= m is written (and read by the adjoint)
 *   power   [planes][lmax]          gpower: the gradient with respect to it, same shape
 * swv2_sht_power: the products on the f32-input MFMA (fp32 accumulation, the k-ordered fma chain), skipping whole 32-row blocks of l
 * below m; per-run partial sums in ws (swv2_sht_ws_bytes), folded by a second launch in ascending order -- no atomics, nothing to zero
 * beforehand, two runs agree bit for bit.  coeffs may be NULL (nothing kept; the forward then writes power and ws only).
 * swv2_sht_adjoint: dX[m][n][k] = sum_{l >= m} table[m][l][k] (2 w_m gpower[plane][l]) c[m][n][l]; every element of dX is written
 * (zeros for m >= lmax).  Refused with SWV2_ERR_INVALID before any launch: a null pointer (coeffs of swv2_sht_power excepted), a
 * non-positive size, planes > 2^20, nlat or lmax > 2^15, mmax > 65535, a workspace smaller than swv2_sht_ws_bytes.  No alignment is
 * asked of any pointer beyond that of a float.  swv2_sht_ws_bytes is host-only and returns 0 for a non-positive argument.
 * swv2_sht_repack: the transposing copy between the layout torch.fft.rfft leaves, F [planes][nlat][mmax][2] (re, im innermost), and the
 * operand layout: X[m][2 p + ri][k] = scale F[p][k][m][ri], or with backward != 0 dst[p][k][m][ri] = scale src[m][2 p + ri][k] (the same
 * map read the other way: the gradient's way back).  Every element of dst is written.  planes <= 65535.
 * swv2_sht_synth: the synthesis, from coefficients back to the longitude transform of a field, with a per-degree response,
 *   S[m][n][k] = rweights[k] sum_{l = m}^{lmax - 1} table[m][l][k] (f_m h(n / 2, l)) coeffs[m][n][l]
 *   f_m = scale_m0 for m = 0, else scale_m;  h(p, l) = response[p response_stride + l], or 1 if response is NULL
 * rweights [nlat] is 1 / w_k of the quadrature weights the table carries (fp32), so rweights[k] table[m][l][k] is the Legendre function
 * itself: the same product as swv2_sht_adjoint on the same table.  response_stride is 0 (one response [lmax] for all planes) or lmax
 * ([planes][lmax]).  S has X's layout and every element is written: zeros for m >= lmax, and exact zeros in the imaginary rows (n odd) of
 * m = 0 and, for an even nlon, of m = nlon / 2, whose coefficients are not read (an inverse real FFT ignores them).  Coefficients with
 * l < m are never read.  No atomics: two runs agree bit for bit.  Refused like swv2_sht_adjoint, and also for a null rweights, another
 * response_stride, nlon < 1. */
size_t swv2_sht_ws_bytes(int planes, int lmax, int mmax);       /* ceil(min(mmax, lmax) / 8) * planes * lmax * 4 */
int swv2_sht_power(const float* table, const float* X, float* power, float* coeffs, int planes, int nlat, int lmax, int mmax, void* ws,
                   size_t ws_bytes, void* stream);
int swv2_sht_adjoint(const float* table, const float* coeffs, const float* gpower, float* dX, int planes, int nlat, int lmax, int mmax,
                     void* stream);
int swv2_sht_repack(const float* src, float* dst, int planes, int nlat, int mmax, float scale, int backward, void* stream);
int swv2_sht_synth(const float* table, const float* rweights, const float* coeffs, const float* response, int response_stride, float scale_m0,
                   float scale_m, float* S, int planes, int nlat, int lmax, int mmax, int nlon, void* stream);

/* Cross spectra of plane pairs (csrc/sht.hip; utils/sht.py: cross_power; purely additive, the revision stays 113).  The operand holds
 * planes = 2 pairs planes in the order a_0, b_0, a_1, b_1, ... (what swv2_sht_repack leaves for fields stacked [pairs][2][nlat][nlon]), so
 * column 4 p + {0, 1, 2, 3} of X[m] is {re a_p, im a_p, re b_p, im b_p}.
 *   spectra  [3][pairs][lmax]   P_aa[p][l] = sum_m w_m |c_a|^2,  P_bb likewise,  C_ab[p][l] = sum_m w_m (re_a re_b + im_a im_b)
 *   gspectra [3][pairs][lmax]   the gradients g_aa, g_bb, g_ab with respect to them
 * swv2_sht_cross_power is swv2_sht_power on the 2 pairs planes with the cross term formed beside the auto terms in the same epilogue: P_aa
 * and P_bb carry the bits swv2_sht_power gives for planes 2 p and 2 p + 1, the coefficients (or NULL) are the same, the partials and the
 * ascending fold work the same way (no atomics, two runs agree bit for bit).
 * swv2_sht_cross_adjoint: dX[m][n][k] = sum_{l >= m} table[m][l][k] ((2 w_m g_self[p][l]) c[m][n][l] + (w_m g_ab[p][l]) c[m][n ^ 2][l]),
 * p = n / 4, g_self = g_aa for n % 4 < 2, else g_bb; per operand element the scales are exact, the partner's product is rounded once and
 * one fma joins the two.  Every element of dX is written (zeros for m >= lmax); coefficients with l < m are never read.
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer (coeffs of the forward excepted), pairs outside 1 .. 32767, the shape
 * limits of swv2_sht_power for 2 pairs planes, a workspace smaller than swv2_sht_cross_ws_bytes (host-only; 0 for a non-positive argument). */
size_t swv2_sht_cross_ws_bytes(int pairs, int lmax, int mmax);   /* ceil(min(mmax, lmax) / 8) * 3 * pairs * lmax * 4 */
int swv2_sht_cross_power(const float* table, const float* X, float* spectra, float* coeffs, int pairs, int nlat, int lmax, int mmax, void* ws,
                         size_t ws_bytes, void* stream);
int swv2_sht_cross_adjoint(const float* table, const float* coeffs, const float* gspectra, float* dX, int pairs, int nlat, int lmax, int mmax,
                           void* stream);

/* First-order conservative regridding to a coarser lat-lon grid (csrc/regrid.hip; utils/regrid.py states the operator and builds the
 * tables; purely additive, the revision stays 113).  All tensors fp32, the tables int32 / fp32, all on the device.
 *   x  C planes of [H][W] per sample, sample b at x + b * x_bstride (elements): a channel block of a wider tensor is read where it lies
 *   y  C planes of [Hd][Wd] per sample, sample b at y + b * y_bstride: it may be a channel block of a wider output
 *   lat_start, lat_count [Hd], lat_w [Hd][KH]: row J of the latitude operator has its weights at the source rows lat_start[J] + k, k < lat_count[J]
 *   lon_start, lon_count [Wd], lon_w [Wd][KW]: row I of the longitude operator, at the source columns (lon_start[I] + k) mod W
 *   r[J][i] = sum_{k < lat_count[J]} lat_w[J][k] x[lat_start[J] + k][i]
 *   y[J][I] = sum_{k < lon_count[I]} lon_w[I][k] r[J][(lon_start[I] + k) mod W]
 * both sums fp32 fma chains from zero with k ascending.  Table entries k >= count are never read, so a NaN or Inf in one source cell
 * reaches exactly the target cells whose bands contain it.  One launch; every element of the C Hd Wd outputs of every sample is
 * written by exactly one thread: no atomics, nothing to zero beforehand, two runs on the same inputs agree bit for bit.
 * The host cannot see the device tables.  The kernel TRUSTS that 1 <= lat_count[J] <= KH, 0 <= lat_start[J], lat_start[J] + lat_count[J] <= H,
 * 1 <= lon_count[I] <= min(KW, W) and 0 <= lon_start[I] < W: the caller guarantees it (utils/regrid.py::Regridder does).
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer, a non-positive size, W % 4 != 0, W > 16384 (the source row is kept in
 * LDS), x not 16-byte aligned, a batch stride that is not a multiple of 4 or (B > 1) smaller than C H W / C Hd Wd, KH or KW outside
 * 1 .. 32, B * C >= 2^20, H * W >= 2^30, Hd * Wd >= 2^30, B * C * ceil(Hd / R) >= 2^31 workgroups (R: the rows per workgroup, 4, 2 or 1).
 * Wd is unrestricted and y needs no alignment beyond a float's. */
int swv2_regrid(const float* x, long x_bstride, float* y, long y_bstride, int B, int C, int H, int W, int Hd, int Wd, const int* lat_start,
                const int* lat_count, const float* lat_w, int KH, const int* lon_start, const int* lon_count, const float* lon_w, int KW,
                void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * ERA5 input assembly (the step BEFORE the model): raw time slabs staged on the device by async H2D copies
 * -> the model's input / target buffers, one pass each.
 *   raw  [B][S][Craw][Hraw][Wraw] fp32   S time slabs per sample as stored in the year files (721 x 1440 rows, uncropped)
 *   out  [B][Cout_total][H][W]    fp32   channels coff .. coff + S*Csel - 1 are written:
 *        out[b][coff + s*Csel + c][i][j] = (raw[b][s][chan[c]][i][j] - mean[c]) / std[c]        i < H, j < W
 * replaces the host-side crop + channel select + z-score of utils/data_loader_era5.py:163-171,98-107 (bit-identical: same
 * operation order, IEEE division) and DALI's fn.normalize (utils/data_loader_era5_dali.py:77-90).
 * swv2_era5_zenith writes nz cos-zenith channels, the per-pixel half of data_loader_era5.py:109-146 (modulus cos_zenith_angle):
 * out[b][coff + k][i][j] = sin(lat_i) sun0 + cos(lat_i) sun1 cos(sun2 + lon_j) on the 0.25 degree grid (lat 90 .. -90, lon 0 ..),
 * sun[(b*nz + k)*3 + {0, 1, 2}] = sin(declination), cos(declination), hour angle at longitude 0 of the time point -- the solar
 * position is float64 host arithmetic (utils/data_loader_era5.py::sun_position; oracle/zenith.py restates the routine);
 * swv2_era5_static broadcasts Cs static feature planes [Cs][H][W] over the batch (utils/preprocess_utils.py:50-68).
 * ------------------------------------------------------------------------------------------------------------ */
int swv2_era5_select_normalize(const float* raw, float* out, const int* chan, const float* mean, const float* stdv, int B, int S,
                               int Csel, int Craw, int Hraw, int Wraw, int H, int W, int Cout_total, int coff, void* stream);
int swv2_era5_zenith(float* out, const float* sun, int B, int nz, int H, int W, int Cout_total, int coff, void* stream);
int swv2_era5_static(const float* stat, float* out, int B, int Cs, int H, int W, int Cout_total, int coff, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * int16-packed year files (utils/packed.py; purely additive, the revision stays 112).  A (year file, channel) is stored as 16-bit codes
 * with one fp32 offset and one fp32 scale:
 *   pack     q  = clamp(rint((x - offset) / scale), -32767, 32767)          q = -32768 for a non-finite x
 *   unpack   xh = (float(q) * scale) + offset                               xh = NaN for q = -32768
 * each step one fp32 operation (no fused multiply-add, IEEE division, round half to even): numpy reproduces every result bit for bit.
 *
 * swv2_era5_select_normalize_i16: swv2_era5_select_normalize with the unpack in front.  raw [B][S][Craw][Hraw][Wraw] int16;
 *   out[b][coff + s*Csel + c][i][j] = (xh - mean[c]) / std[c], xh unpacked with offset / scale[slab_row[b*S + s] * Craw + chan[c]]:
 *   offset, scale are tables [rows][Craw] fp32 of every year file's parameters, slab_row [B][S] int32 names the row of each slab, so the
 *   samples of one batch may come from different years.  Equal, bit for bit, to swv2_era5_select_normalize on the unpacked slab.
 * swv2_era5_unpack_i16 / swv2_era5_pack_i16: a whole slab [C][H][W] with one parameter row offset [C], scale [C].
 * swv2_pack_range: per-channel minimum and maximum of the finite values of slab [C][H][W] fp32 and the number of the others, folded into
 *   the running range [C][2] fp32 (min, max) and missing [C] int64 of a year file; first != 0 overwrites them.  A channel without a
 *   finite value so far holds (+inf, -inf).  Minima, maxima and counts do not depend on order: two runs agree bit for bit.  ws: at least
 *   swv2_pack_range_ws_bytes(C, H, W) bytes (host-only; 0 for a non-positive size), not zeroed by the caller.
 * Refused with SWV2_ERR_INVALID before any launch: a null pointer, a non-positive size, W % 4 or Wraw % 4 != 0, H > Hraw, W > Wraw, an
 * int16 pointer not 8-byte aligned, an fp32 slab / out pointer not 16-byte aligned, a channel range outside the output, more than 65535
 * planes in one call (C of a slab; B * S * Csel), H * W >= 2^30, ws / missing not 8-byte aligned, a workspace smaller than its _ws_bytes.
 * ------------------------------------------------------------------------------------------------------------ */
int swv2_era5_select_normalize_i16(const int16_t* raw, float* out, const int* chan, const float* mean, const float* stdv, const float* offset,
                                   const float* scale, const int* slab_row, int B, int S, int Csel, int Craw, int Hraw, int Wraw, int H, int W,
                                   int Cout_total, int coff, void* stream);
int swv2_era5_unpack_i16(const int16_t* raw, float* out, const float* offset, const float* scale, int C, int H, int W, void* stream);
int swv2_era5_pack_i16(const float* slab, int16_t* out, const float* offset, const float* scale, int C, int H, int W, void* stream);
size_t swv2_pack_range_ws_bytes(int C, int H, int W);     /* C * slices of the plan * 16 */
int swv2_pack_range(const float* slab, int C, int H, int W, int first, float* range, int64_t* missing, void* ws, size_t ws_bytes, void* stream);

/* Output projection of the attention branch fused with LayerNorm1 (swinv2_global.py:318-319, 468-476, 490):
 *   forward : y[dst] = x[dst] + scale[b] * LN(merge_heads(oh) Wp^T + bp),  dst = rowidx[m] (negative = padded row, skipped);
 *             saves a1 = bf16(proj output) [Bw*Lp][C] (window order), mean, rstd            (replaces swv2_linear + swv2_ln_residual_fwd)
 *   backward: da1 = LN backward of scale * dy[dst] (zeros for padded rows), d(oh) = split_heads(da1 Wp), head-major;
 *             dgamma / dbeta ACCUMULATED; ws >= swv2_proj_ln_bwd_ws_floats(Bw*Lp, C) floats   (replaces swv2_ln_residual_bwd + swv2_linear)
 * C in {32,64,96,128}, head dim padded to 16, an even number of heads with heads * 16 <= 128; or C = 192 with up to 8 heads in
 * 32-wide slots (oh / doh [Bw][heads][Lp][32], wp [192][heads*32], wpt [heads*32][192]: BASELINE configs[4])  (swv2_proj_ln_supported).
 * Lp % 16 == 0.  Anything else is refused with a non-zero return before any launch; nothing is written.
 * Padded rows (rowidx[m] < 0): a1, mean and rstd are computed and stored like those of any other row (from whatever oh holds
 * there: the attention kernels leave zeros, so a1 = bf16(bp)); only their y row is skipped.  The backward reads them (they must
 * be finite), writes da1 = +0 and d(oh) = 0 on these rows -- the proj weight gradient relies on it -- and counts them in neither
 * dgamma nor dbeta.  The padded head columns of d(oh) are 0 (zero rows of wpt).  Rows past Bw*Lp in a ragged last row tile are
 * clamped to the last row: nothing outside the tensors is written and the last row counts once.
 * scale[b]: b = dst / rows_per_sample of the DESTINATION row and nothing more; rows_per_sample need not divide the row count,
 * Lp, the valid rows of a window or a tile height.  y rows that no table entry names are not written.
 * Both directions are bit-reproducible.  Per-element accuracy: tests/test_proj_ln_exact_gpu.py (bounds: tests/proj_ln_reference.py). */
typedef struct {
    const void* oh;        /* bf16 [Bw][heads][Lp][16] */
    const void* wp;        /* bf16 [C][heads*16] (swv2_prep_weight with the head-padding column map) */
    const float* bp;       /* [C] */
    const float* gamma; const float* beta; const float* scale;
    const int32_t* rowidx; /* [Bw*Lp] or NULL (identity) */
    const float* x;        /* fp32 [rows][C] residual, destination order */
    void* a1; float* mean; float* rstd;     /* out, window order: bf16 [Bw*Lp][C], [Bw*Lp], [Bw*Lp]; every row, padded ones included */
    float* y;              /* out fp32 [rows][C], destination order */
    int Bw, Lp, heads, C, rows_per_sample;
    float eps;
} swv2_proj_ln_args;
typedef struct {
    const float* dy;       /* fp32 [rows][C] gradient of y, destination order */
    const void* a1; const float* mean; const float* rstd; const float* gamma; const float* scale;
    const int32_t* rowidx;
    const void* wpt;       /* bf16 [heads*16][C] = proj.weight^T (swv2_prep_weight, transpose, head-padding row map) */
    void* da1;             /* out bf16 [Bw*Lp][C]; +0 on padded rows */
    void* doh;             /* out bf16 [Bw][heads][Lp][16] */
    float* dgamma; float* dbeta; float* ws;
    int Bw, Lp, heads, C, rows_per_sample;
} swv2_proj_ln_bwd_args;
int swv2_proj_ln_supported(int C, int heads, int head_pad);
size_t swv2_proj_ln_bwd_ws_floats(int Mw, int C);
int swv2_proj_ln_fwd(const swv2_proj_ln_args* a, void* stream);
int swv2_proj_ln_bwd(const swv2_proj_ln_bwd_args* a, void* stream);

/* Fused MLP branch, forward: y = x + scale[b] * LayerNorm(fc2(GELU(fc1(x))))  (swinv2_global.py:492-496, timm Mlp
 * :381-386) in one kernel; the [M][hidden] activation stays in registers.  Saves for the backward: hpre = bf16(fc1(x)),
 * a2 = bf16(fc2 output), mean / rstd of the LayerNorm.  Same results as swv2_linear(EPI_BF16_GELU) + swv2_linear +
 * swv2_ln_residual_fwd (identical rounding points).  C in {32,64,96,128,192,256}, hidden % 32 == 0,
 * hidden <= 2048 (swv2_mlp_supported); other shapes return SWV2_ERR_UNSUPPORTED -- use the unfused sequence.
 * Contracts (pinned element by element by tests/test_mlp_exact_gpu.py; they hold for swv2_mlp_bwd as well):
 *   - nothing outside rows 0 .. M-1 of an output is written, whatever M is (1 included): a row tile's rows past M are computed as
 *     copies of row M-1 and stored to row M-1 again (same values), and count once in dgamma / dbeta;
 *   - rows_per_sample is any positive number: it need not divide M, a row tile or a workgroup's rows;
 *   - a refused call (non-zero return: unsupported C / hidden, M <= 0, rows_per_sample <= 0, a missing pointer) writes nothing;
 *   - GELU and GELU' are taken of the STORED bf16 pre-activation.  For 2^-14 <= |x| < 16 they come from a table each workgroup
 *     fills with the fp32 formulas (the backward at C = 192 holds the positive half and uses GELU'(-x) = 1 - GELU'(x); at C = 256
 *     it evaluates the formula); +-0, |x| < 2^-14, |x| >= 16 and non-finite arguments take the formula, together with the other
 *     values of their 16-row x 16-hidden-unit tile.  Either way the activation fed to fc2 is bit for bit the bf16(GELU) that
 *     SWV2_OP_BF16_GELU / SWV2_EPI_BF16_GELU produce for the same stored value;
 *   - results are deterministic: a second call gives the same bits in every output, dgamma / dbeta and ws included;
 *   - the mode that keeps no pre-activation (hpre == NULL here, recompute mode in swv2_mlp_bwd) gives bit for bit the outputs of
 *     the mode that keeps it. */
typedef struct {
    const float* x;        /* [M][C] fp32 rows: GEMM input and residual */
    const void* w1;        /* bf16 [hidden][C]  (swv2_prep_weight) */
    const float* b1;       /* [hidden] */
    const void* w2;        /* bf16 [C][hidden] */
    const float* b2;       /* [C] */
    const float* gamma;    /* LayerNorm weight / bias [C] */
    const float* beta;
    const float* scale;    /* per-sample drop-path factor [M / rows_per_sample] or NULL */
    void* hpre;            /* out bf16 [M][hidden], or NULL: not kept (the backward then runs in recompute mode) */
    void* a2;              /* out bf16 [M][C] */
    float* mean;           /* out [M] */
    float* rstd;
    float* y;              /* out fp32 [M][C] */
    int M, C, hidden, rows_per_sample;
    float eps;
} swv2_mlp_args;
int swv2_mlp_supported(int C, int hidden);
int swv2_mlp_recompute_supported(int C, int hidden);      /* the backward's recompute mode (swv2_mlp_bwd_args.hpre == NULL) */
int swv2_mlp_fwd(const swv2_mlp_args* a, void* stream);

/* Fused MLP branch, backward (the autograd of swv2_mlp_fwd w.r.t. x and the data-path intermediates):
 *   da2 = LayerNorm backward of scale[b] * dy (saved a2, mean, rstd);  dh = (da2 W2) * GELU'(hpre);  dx = dy + dh W1
 * in one kernel (replaces swv2_ln_residual_bwd + swv2_linear(EPI_GELU_GRAD) + swv2_linear(EPI_F32)).  da2 and dh are
 * written for the weight gradients (swv2_linear_wgrad: d fc2 = da2^T GELU(hpre), d fc1 = dh^T x).  dgamma / dbeta are
 * ACCUMULATED.  ws: >= swv2_mlp_bwd_ws_floats(M, C) floats, contents undefined afterwards. */
typedef struct {
    const float* dy;       /* [M][C] gradient of y */
    const void* a2;        /* bf16 [M][C]      saved by the forward */
    const float* mean;     /* [M] */
    const float* rstd;
    const float* gamma;    /* [C] */
    const float* scale;    /* per-sample drop-path factor or NULL */
    const void* hpre;      /* bf16 [M][hidden] saved by the forward, or NULL (recompute mode, below) */
    const void* w2t;       /* bf16 [hidden][C] = fc2.weight^T (swv2_prep_weight, transpose) */
    const void* w1t;       /* bf16 [C][hidden] = fc1.weight^T */
    void* da2;             /* out bf16 [M][C] */
    void* dh;              /* out bf16 [M][hidden] */
    float* dx;             /* out fp32 [M][C] */
    float* dgamma;         /* [C], accumulated */
    float* dbeta;
    float* ws;
    int M, C, hidden, rows_per_sample;
    /* recompute mode (hpre == NULL; w1t unused): the pre-activation is rebuilt from the forward's input instead of read back
     * -- the forward (swv2_mlp_args.hpre == NULL) then never writes it: 16 bytes per token-channel less per block */
    const float* x;        /* [M][C] the forward's input */
    const void* w1;        /* bf16 [hidden][C] fc1.weight */
    const float* b1;       /* [hidden] */
} swv2_mlp_bwd_args;
size_t swv2_mlp_bwd_ws_floats(int M, int C);
int swv2_mlp_bwd(const swv2_mlp_bwd_args* a, void* stream);

/* Continuous position bias (swinv2_global.py:240-261,274-287): bias[heads][L][L] = meta_mlp(log-spaced relative
 * coordinates), meta_mlp = Linear(2,hidden) -> ReLU -> Dropout(drop_p) -> Linear(hidden,heads); the relative-coordinate
 * table is generated in-kernel.  keep_bf16: [L*L][hidden] keep-mask drawn by the caller (any non-zero = keep; the kernel
 * applies 1/(1-drop_p)), NULL in eval mode.  Backward outputs are ACCUMULATED (caller zeroes). */
int swv2_cpb_fwd(const float* w1, const float* b1, const float* w2, const float* b2, const void* keep_bf16, float* bias,
                 int wh, int ww, int heads, int hidden, float drop_p, void* stream);
int swv2_cpb_bwd(const float* dbias, const float* w1, const float* b1, const float* w2, const void* keep_bf16, float* dw1,
                 float* db1, float* dw2, float* db2, int wh, int ww, int heads, int hidden, float drop_p, void* stream);
/* The same with a caller workspace of swv2_cpb_bwd_ws_bytes(wh, ww, heads, hidden) bytes: every workgroup leaves one partial row,
 * a second launch adds them in a fixed order -- no float atomics (bit-reproducible gradients).  ws = NULL: the atomics
 * path of swv2_cpb_bwd.  A non-NULL ws of fewer bytes is an error (SWV2_ERR_INVALID, nothing launched, nothing written), not a silent
 * switch to the atomics.  Outputs ACCUMULATED as above. */
size_t swv2_cpb_bwd_ws_bytes(int wh, int ww, int heads, int hidden);
int swv2_cpb_bwd_ws(const float* dbias, const float* w1, const float* b1, const float* w2, const void* keep_bf16, float* dw1,
                    float* db1, float* dw2, float* db2, int wh, int ww, int heads, int hidden, float drop_p, void* ws,
                    size_t ws_bytes, void* stream);

/* The tables of ALL blocks of a stage in one launch each way (nothing in :240-261,274-287 depends on activations, so the model
 * computes the `nblk` tables before its first block and their parameter gradients after the first block's backward).
 *   params_dev : DEVICE array [nblk][4] of device pointers: w1 [hidden][2], b1 [hidden], w2 [heads][hidden], b2 [heads] of each block
 *   keep_bits  : u32 [nblk][L*L][hidden / 8] of uniformly random bits drawn by the caller (31 random bits per word are enough: only the
 *                three low bytes are used), or NULL (eval).  Hidden unit j of a pair <-> bit (j & 7) of W | W >> 8 | W >> 16 with
 *                W = word ((j >> 3) & 3) * (hidden / 32) + (j >> 5) of the pair: the unit is DROPPED iff that bit is clear in all three
 *                low bytes of W -- probability 1/8, the reference's hard-coded Dropout(0.125) (:245; drop_p must be 0.125); kept units
 *                are scaled by 1 / (1 - drop_p)
 *   bias       : out [nblk][heads][L][L]
 * backward: dbias_tables [nblk][nchunk][heads][L][L] -- d bias of a block = the SUM of its nchunk tables (the per-workgroup tables
 * swv2_attn_bwd leaves with dbias_partials; nchunk = 1: plain gradients) -- grads [nblk][3 hidden + heads hidden + heads] =
 * (dw1 | db1 | dw2 | db2) per block, ACCUMULATED; ws: swv2_cpb_bwd_multi_ws_bytes.  heads <= 16, hidden in {64, 128, 256, 384, 512}.  No atomics;
 * both directions run their contractions on the matrix pipe with hi + lo split bf16 operands (fp32 accuracy: ~1e-5 relative). */
int swv2_cpb_fwd_multi(const float* const* params_dev, int nblk, const uint32_t* keep_bits, float* bias, int wh, int ww, int heads,
                       int hidden, float drop_p, void* stream);
size_t swv2_cpb_bwd_multi_ws_bytes(int nblk, int wh, int ww, int heads, int hidden);
int swv2_cpb_bwd_multi(const float* dbias_tables, int nchunk, const float* const* params_dev, int nblk, const uint32_t* keep_bits,
                       float* grads, int wh, int ww, int heads, int hidden, float drop_p, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Whole-block orchestration: one host call enqueues every launch of a Swin block (reference
 * SwinTransformerV2CrBlock.forward, swinv2_global.py:480-497, and its autograd) from C++, so the per-launch host cost is a few
 * microseconds instead of a Python round trip.  Which launches those are is decided by swv2_block_plan (below the descriptor) and
 * by nothing else: 4 forward / 5 backward steps with every fusion, 7 / 11 with none.  All memory is caller-owned.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct swv2_block_desc {
    /* geometry */
    int B, T, C, heads, head_dim, hidden, L, Lp, DP, nwh, nww, mask_thr;
    const int32_t* rowidx;   /* [Bw*Lp] window-ordered padded row -> image row (b*T + i*gw + j) or -1 */
    const int32_t* qkv_map;  /* [3*heads*DP] padded qkv feature -> qkv feature or -1 */
    const int32_t* proj_map; /* [heads*DP]   padded head feature -> channel or -1 */
    /* parameters (fp32) and their prepared bf16 copies (swv2_prep_weight) */
    const float *logit_scale, *qkv_b_pad, *proj_b, *n1_w, *n1_b, *fc1_b, *fc2_b, *n2_w, *n2_b;
    const void *w_qkv, *w_proj, *w_fc1, *w_fc2;     /* forward: [3hDP][C], [C][hDP], [hid][C], [C][hid] */
    const void *w_qkvt, *w_projt, *w_fc1t, *w_fc2t; /* backward (transposed): [C][3hDP], [hDP][C], [C][hid], [hid][C] */
    /* per-call inputs */
    const float* x;          /* [B*T][C] block input (residual stream) */
    const float* bias;       /* [heads][L][L] CPB table or NULL */
    void* bias_pack;         /* with bias: swv2_attn_pack_bias_bytes(heads, L) bytes, written by the forward, read by both */
    const float* dp1;        /* [B] drop-path scales or NULL */
    const float* dp2;
    /* saved activations: written by forward, read by backward */
    void* qkvh;  float* rnorm; void* oh; float* lse; void* a1; float* mean1; float* rstd1; float* x1;
    void* hpre;  void* hact;   void* a2; float* mean2; float* rstd2;      /* hact: need_hact_bytes of the plan (may be NULL at 0) */
    float* x2;               /* forward output [B*T][C] */
    /* backward only */
    const float* dx2;        /* grad of x2 */
    void *da2, *dh, *da1, *doh, *dqkvh;   /* bf16 scratch: [BT][C], [BT][hid], [Bw*Lp][C], [Bw][h][Lp][DP], [Bw][h][3][Lp][DP] */
    float* dx1;              /* fp32 scratch [BT][C] */
    float* ln_ws;            /* ln_ws_floats floats, at least max(SWV2_LN_BWD_MAX_BLOCKS*2*C, swv2_mlp_bwd_ws_floats(B*T, C),
                                swv2_proj_ln_bwd_ws_floats(Bw*Lp, C)); need_ln_ws_floats of the plan for one fold of both LayerNorms */
    float* dx;               /* out: grad of x */
    /* parameter gradients, ACCUMULATED (caller zeroes) */
    float *d_logit_scale, *d_bias, *d_qkv_w, *d_qkv_b, *d_proj_w, *d_proj_b, *d_n1_w, *d_n1_b, *d_fc1_w, *d_fc1_b,
          *d_fc2_w, *d_fc2_b, *d_n2_w, *d_n2_b;
    int wgrad_splits;        /* row slices of the single weight-gradient products (0 = 64) */
    /* optional timing of ONE launch with HIP events on the launch stream (bench.py's roofline): if ev_kernel matches the
       launch id of a step of the plan (swv2_block_step_id: forward 1 qkv, 2 attn_fwd, 3 proj, 4 ln1, 5 fc1, 6 fc2, 7 ln2; backward
       11 ln2, 12 wgrad fc2, 13 dh, 14 wgrad fc1, 15 dx1, 16 ln1, 17 wgrad proj, 18 d(oh), 19 attn_bwd, 20 wgrad qkv, 21 dx, 22 grouped
       weight gradients; a fused kernel answers to the id of the first launch it replaces), ev_start / ev_stop (hipEvent_t) are
       recorded around it; 0 = off */
    int ev_kernel;
    void* ev_start;
    void* ev_stop;
    /* requests; what runs is swv2_block_plan's answer */
    int fuse_proj_ln;        /* 1: proj + LN1 run as swv2_proj_ln_fwd / _bwd when the shape is supported */
    int fuse_mlp;            /* 1: fc1, fc2 and LN2 run as swv2_mlp_fwd / _bwd when the shape is supported (hact is then neither
                                written nor read: the backward applies GELU to hpre on load) */
    void* wgrad_ws;          /* optional workspace of the weight-gradient products (swv2_linear_wgrad_ws), shared by the four
                                products of the block (they are ordered on one stream); NULL = atomic accumulation */
    size_t wgrad_ws_bytes;
    int wgrad_group;         /* 1 (with the fused MLP path and a workspace of swv2_block_wgrad_ws_bytes): the four products run as ONE
                                swv2_block_wgrad launch at the end of the backward (launch id 22) */
    void* grad_zero;         /* optional: one buffer holding all 13 parameter gradients of the block (16-byte aligned, a multiple
                                of 16 bytes); where the plan says grad_zero_in_kernel the backward's first kernel zeroes it, so the
                                caller need not (otherwise, and with NULL, the caller zeroes every d_* buffer itself) */
    size_t grad_zero_bytes;
    size_t ln_ws_floats;     /* floats available at ln_ws; >= swv2_mlp_bwd_ws_floats + swv2_proj_ln_bwd_ws_floats lets the backward
                                keep both LayerNorms' d gamma / d beta partial rows and fold them with ONE launch (0: one each) */
    int bias_prepacked;      /* 1: bias_pack already holds the packed table (swv2_attn_pack_bias_multi: all blocks' tables in one
                                launch before the first block); 0: swv2_block_fwd packs `bias` into bias_pack itself */
    float* dbias_part;       /* optional, with bias: swv2_attn_dbias_ws_bytes(heads, L, swv2_attn_bias_chunks(Bw)) bytes.  The backward
                                LEAVES the attention workgroups' d bias tables there (swv2_attn_args.dbias_partials) and does not
                                touch d_bias (may be NULL): the caller sums them with swv2_cpb_bwd_multi */
    size_t dbias_part_bytes;
} swv2_block_desc;

/* The launch plan of a block: THE place where its launches are decided.  swv2_block_fwd / swv2_block_bwd compute it per call and run
 * its step lists, one launch per step, so what they enqueue is what it says.  Host arithmetic with no launch; the one HIP call is
 * in wgrad_kernel of a grouped plan, where swv2_block_wgrad_kernel asks for the current device's CU count (256 in a process without
 * a GPU) -- swv2_block_fwd / _bwd skip that field, which no launch depends on.  It reads from the descriptor: the geometry; the requests fuse_mlp, fuse_proj_ln,
 * wgrad_group, wgrad_splits; bias, bias_pack, dbias_part, grad_zero and wgrad_ws for PRESENCE (no pointer is dereferenced; a NULL
 * wgrad_ws counts as 0 bytes); bias_prepacked; the capacities ln_ws_floats and wgrad_ws_bytes.  A caller sizes its buffers by
 * filling geometry and requests, reading the three need_* fields (they do not depend on the capacities), and calling again with the
 * capacities it provides: a capacity below the need is legal and only loses the decision that needs it. */
enum swv2_block_step {       /* forward */
    SWV2_STEP_RNORM_ZERO = 1,    /* DP > 64: memset of rnorm (the qkv epilogue accumulates squared norms there)       */
    SWV2_STEP_QKV,               /* roll + partition gather | qkv GEMM | + bias, split heads, (DP <= 64) L2-normalise */
    SWV2_STEP_QK_NORMALIZE,      /* DP > 64: swv2_qk_normalize                                                        */
    SWV2_STEP_PACK_BIAS,         /* a table that is not prepacked: swv2_attn_pack_bias into bias_pack                 */
    SWV2_STEP_ATTN_FWD,
    SWV2_STEP_PROJ, SWV2_STEP_LN1_FWD,
    SWV2_STEP_PROJ_LN_FWD,       /* the two above as swv2_proj_ln_fwd                                                 */
    SWV2_STEP_FC1, SWV2_STEP_FC2, SWV2_STEP_LN2_FWD,
    SWV2_STEP_MLP_FWD,           /* the three above as swv2_mlp_fwd                                                   */
    /* backward */
    SWV2_STEP_LN2_BWD, SWV2_STEP_WGRAD_FC2, SWV2_STEP_DH, SWV2_STEP_WGRAD_FC1, SWV2_STEP_DX1,
    SWV2_STEP_MLP_BWD,           /* LN2_BWD + DH + DX1 as swv2_mlp_bwd                                                */
    SWV2_STEP_LN1_BWD,
    SWV2_STEP_PROJ_LN_BWD,       /* LN1_BWD + DOH as swv2_proj_ln_bwd                                                 */
    SWV2_STEP_WGRAD_PROJ, SWV2_STEP_DOH, SWV2_STEP_ATTN_BWD, SWV2_STEP_WGRAD_QKV, SWV2_STEP_DX,
    SWV2_STEP_LN_FOLD,           /* deferred, not grouped: both LayerNorms' partial rows -> d gamma / d beta, one launch */
    SWV2_STEP_WGRAD_GROUP,       /* the four WGRAD_* as swv2_block_wgrad (+ the deferred fold riding on its reduction)  */
    SWV2_STEP_COUNT
};
#define SWV2_BLOCK_MAX_STEPS 12
enum { SWV2_DBIAS_NONE = 0,      /* no CPB table                                                                              */
       SWV2_DBIAS_ATOMICS = 1,   /* no workspace at all: float atomics on d_bias                                              */
       SWV2_DBIAS_WGRAD_WS = 2,  /* wgrad_ws (idle at that point) is lent to swv2_attn_bwd as dbias_ws, one more launch sums
                                    into d_bias; a workspace too small for the tables: atomics (swv2_attn_args.dbias_ws)      */
       SWV2_DBIAS_PART = 3 };    /* left in dbias_part for the caller to sum (swv2_cpb_bwd_multi); d_bias untouched           */
typedef struct swv2_block_plan_t {
    /* decisions */
    int mlp_fused;               /* fuse_mlp && swv2_mlp_supported                                                            */
    int proj_ln_fused;           /* fuse_proj_ln && swv2_proj_ln_supported                                                    */
    int ln_deferred;             /* both fused and ln_ws_floats >= swv2_mlp_bwd_ws_floats + swv2_proj_ln_bwd_ws_floats: both
                                    LayerNorms' partial rows are kept and folded once (otherwise each kernel folds its own)   */
    int wgrad_grouped;           /* wgrad_group, MLP fused and wgrad_ws_bytes >= swv2_block_wgrad_ws_bytes(C, hidden, heads*DP, 0) */
    int wgrad_kernel;            /* grouped: swv2_block_wgrad_kernel's answer (SWV2_BLOCK_WGRAD_*) for it; else -1            */
    int grad_zero_in_kernel;     /* grad_zero offered and MLP fused: the backward's first kernel zeroes it                    */
    int attn_fwd_chunks, attn_bwd_chunks;   /* swv2_attn_args.max_chunks of the two attention launches                        */
    int dbias_dest;              /* SWV2_DBIAS_*                                                                              */
    /* what the caller provides for the full plan */
    size_t need_hact_bytes;      /* 0 when the MLP branch is fused                                                            */
    size_t need_ln_ws_floats;
    size_t need_wgrad_ws_bytes;  /* the largest of the four swv2_linear_wgrad_ws_bytes and, with wgrad_group, swv2_block_wgrad_ws_bytes */
    /* the steps each direction enqueues, in order */
    int n_fwd, n_bwd;
    int fwd[SWV2_BLOCK_MAX_STEPS], bwd[SWV2_BLOCK_MAX_STEPS];
} swv2_block_plan_t;
int swv2_block_plan(const swv2_block_desc* d, swv2_block_plan_t* out);
/* launch id of a step (the value swv2_block_desc.ev_kernel names it by; 0: never bracketed; -1: no such step) and its name */
int swv2_block_step_id(int step);
const char* swv2_block_step_name(int step);

int swv2_block_fwd(const swv2_block_desc* d, void* stream);
int swv2_block_bwd(const swv2_block_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWV2_H */
