// Host-side orchestration of one Swin block on top of the public kernels' entry points.  swv2_block_plan decides ONCE which launches a
// block runs (fused or separate kernels, one LayerNorm fold or two, grouped weight gradients, workspace needs); swv2_block_fwd /
// swv2_block_bwd execute its step lists: with every fusion 4 forward steps (qkv, attention, proj + LN1, MLP) and 5 backward steps (MLP,
// proj + LN1, attention, dx, the grouped weight gradients), without any 7 and 11.  Pure C++ host code: no device code here, no
// allocation, no synchronisation, no state kept between calls.
#include "common.h"

namespace {

swv2_operand op(int kind, const void* p, int rows, int cols, long ld, const int32_t* rowidx = nullptr) {
    swv2_operand o = {};
    o.kind = kind; o.ptr = p; o.rowidx = rowidx; o.ld = ld; o.rows = rows; o.cols = cols;
    return o;
}
swv2_operand op_heads(const void* p, int Bw, int heads, int parts, int Lp, int DP) {
    swv2_operand o = op(SWV2_OP_HEADS, p, Bw * Lp, parts * heads * DP, parts);
    o.p[0] = heads; o.p[2] = Lp; o.p[3] = DP;
    return o;
}
swv2_epilogue epi(int kind, void* out, long ld, const float* bias = nullptr, const void* aux = nullptr,
                  float* aux_out = nullptr, const int32_t* rowidx = nullptr) {
    swv2_epilogue e = {};
    e.kind = kind; e.out = out; e.ld = ld; e.bias = bias; e.aux = aux; e.aux_out = aux_out; e.rowidx = rowidx;
    return e;
}
swv2_attn_args attn(const swv2_block_desc* d, int max_chunks) {
    swv2_attn_args a = {};
    a.qkvh = d->qkvh; a.logit_scale = d->logit_scale; a.bias = d->bias; a.bias_pack = d->bias ? d->bias_pack : nullptr;
    a.oh = d->oh; a.lse = d->lse;
    a.Bw = d->B * d->nwh * d->nww; a.heads = d->heads; a.L = d->L; a.head_dim = d->head_dim; a.nwh = d->nwh; a.nww = d->nww;
    a.mask_thr = d->mask_thr; a.max_chunks = max_chunks;
    return a;
}
// the block's four weight-gradient products (0 fc2, 1 fc1, 2 proj, 3 qkv; the item order of swv2_block_wgrad), described ONCE: the single
// launches and the grouped launch of swv2_block_bwd read the same items.  fused: the fused MLP path stores no hact, fc2's X operand is
// GELU(hpre) on load
void wgrad_items(const swv2_block_desc* d, bool fused, swv2_wgrad_item it[4]) {
    const int BT = d->B * d->T, Bw = d->B * d->nwh * d->nww, Mw = Bw * d->Lp, C = d->C, h = d->heads, hid = d->hidden;
    it[0].dy = op(SWV2_OP_BF16, d->da2, BT, C, C);
    it[0].x = fused ? op(SWV2_OP_BF16_GELU, d->hpre, BT, hid, hid) : op(SWV2_OP_BF16, d->hact, BT, hid, hid);
    it[0].dW = d->d_fc2_w; it[0].db = d->d_fc2_b; it[0].ldw = hid;
    it[1].dy = op(SWV2_OP_BF16, d->dh, BT, hid, hid); it[1].x = op(SWV2_OP_F32, d->x1, BT, C, C);
    it[1].dW = d->d_fc1_w; it[1].db = d->d_fc1_b; it[1].ldw = C;
    it[2].dy = op(SWV2_OP_BF16, d->da1, Mw, C, C); it[2].x = op_heads(d->oh, Bw, h, 1, d->Lp, d->DP);
    it[2].dW = d->d_proj_w; it[2].db = d->d_proj_b; it[2].kmap = d->proj_map; it[2].ldw = C;
    it[3].dy = op_heads(d->dqkvh, Bw, h, 3, d->Lp, d->DP); it[3].x = op(SWV2_OP_F32, d->x, Mw, C, C, d->rowidx);
    it[3].dW = d->d_qkv_w; it[3].db = d->d_qkv_b; it[3].nmap = d->qkv_map; it[3].ldw = C;
}
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// every step of the plans: the launch id bench.py's per-kernel timing asks for through swv2_block_desc.ev_kernel (0 = never bracketed; a
// fused kernel shares the id of the first launch it replaces) and the name swin_v2_weather_amd/ops.py::BLOCK_KERNEL_IDS knows it by
const struct { int id; const char* name; } STEPS[SWV2_STEP_COUNT] = {
    {0, "end"},
    {0, "rnorm_zero"}, {1, "qkv"}, {0, "qk_normalize"}, {0, "pack_bias"}, {2, "attn_fwd"}, {3, "proj"}, {4, "ln1_fwd"}, {3, "proj_ln_fwd"},
    {5, "fc1"}, {6, "fc2"}, {7, "ln2_fwd"}, {5, "mlp_fwd"},
    {11, "ln2_bwd"}, {12, "wgrad_fc2"}, {13, "dh"}, {14, "wgrad_fc1"}, {15, "dx1"}, {13, "mlp_bwd"}, {16, "ln1_bwd"}, {16, "proj_ln_bwd"},
    {17, "wgrad_proj"}, {18, "doh"}, {19, "attn_bwd"}, {20, "wgrad_qkv"}, {21, "dx"}, {0, "ln_fold"}, {22, "wgrad_group"},
};
static_assert(SWV2_STEP_WGRAD_GROUP + 1 == SWV2_STEP_COUNT && SWV2_STEP_MLP_FWD == 12 && SWV2_STEP_LN2_BWD == 13, "STEPS follows enum swv2_block_step");

// launch `x` as step `step` (one with a launch id); bracket it with the caller's HIP events when it is the one being timed
#define LAUNCH(step, x)                                                                                     \
    do {                                                                                                    \
        const bool t_ = d->ev_kernel == STEPS[step].id && d->ev_start && d->ev_stop;                         \
        if (t_) (void)hipEventRecord((hipEvent_t)d->ev_start, (hipStream_t)st);                             \
        TRY(x);                                                                                             \
        if (t_) (void)hipEventRecord((hipEvent_t)d->ev_stop, (hipStream_t)st);                              \
    } while (0)

// THE place where a block's launches are decided: everything of swv2_block_plan_t except wgrad_kernel, which no launch depends on
// (swv2_block_plan adds it).  Reads geometry, switches, pointers for presence and the two capacities; arithmetic only, no HIP call
int plan_block(const swv2_block_desc* d, swv2_block_plan_t* p) {
    SWV2_CHECK_ARG(d && p, "swv2_block_plan: null descriptor or plan");
    SWV2_CHECK_ARG(d->B > 0 && d->T > 0 && d->C > 0 && d->heads > 0 && d->hidden > 0 && d->Lp > 0 && d->DP > 0 && d->nwh > 0 && d->nww > 0,
                   "swv2_block_plan: non-positive geometry");
    *p = {};
    const int BT = d->B * d->T, Bw = d->B * d->nwh * d->nww, Mw = Bw * d->Lp, C = d->C, h = d->heads, hid = d->hidden;
    const int sp = d->wgrad_splits > 0 ? d->wgrad_splits : 64;
    const size_t ws_bytes = d->wgrad_ws ? d->wgrad_ws_bytes : 0;
    const size_t ln_pair = swv2_mlp_bwd_ws_floats(BT, C) + swv2_proj_ln_bwd_ws_floats(Mw, C);
    // what the caller provides for the full plan: the GELU output only where fc2 reads it back; both LayerNorms' partial rows side by
    // side; the largest of the four single products' workspaces and (when asked for) the grouped launch's
    p->need_ln_ws_floats = std::max((size_t)SWV2_LN_BWD_MAX_BLOCKS * 2 * C, ln_pair);
    p->need_wgrad_ws_bytes = d->wgrad_group ? swv2_block_wgrad_ws_bytes(C, hid, h * d->DP, 0) : 0;
    const int prod[4][3] = {{BT, C, hid}, {BT, hid, C}, {Mw, C, h * d->DP}, {Mw, 3 * h * d->DP, C}};        // (rows, N, K)
    for (const auto& q : prod)
        p->need_wgrad_ws_bytes = std::max(p->need_wgrad_ws_bytes, swv2_linear_wgrad_ws_bytes(q[0], q[1], q[2], sp));

    p->mlp_fused = d->fuse_mlp && swv2_mlp_supported(C, hid);
    p->proj_ln_fused = d->fuse_proj_ln && swv2_proj_ln_supported(C, h, d->DP);
    p->need_hact_bytes = p->mlp_fused ? 0 : (size_t)BT * hid * 2;
    // both LayerNorms' d gamma / d beta partial rows kept and folded once: needs both fused kernels and room for both sets of rows
    p->ln_deferred = p->mlp_fused && p->proj_ln_fused && d->ln_ws_floats >= ln_pair;
    // the four weight gradients as ONE launch after the data path (needs the fused MLP path's operand set: GELU(hpre) on load; the
    // proj + LN1 pair may be fused or not)
    p->wgrad_grouped = d->wgrad_group && p->mlp_fused && d->wgrad_ws && ws_bytes >= swv2_block_wgrad_ws_bytes(C, hid, h * d->DP, 0);
    p->wgrad_kernel = -1;
    // all parameter gradients in one buffer: the fused MLP backward, the first kernel of the backward, zeroes it on the side
    p->grad_zero_in_kernel = p->mlp_fused && d->grad_zero != nullptr;
    // forward with a table: per-workgroup table load -- fewer, longer-lived workgroups
    p->attn_fwd_chunks = d->bias ? 32 : 64;
    p->attn_bwd_chunks = 64;
    if (d->bias) {
        // every workgroup adds its d bias table with atomics: fewer, longer-lived workgroups (end-to-end at depth 12:
        // 16 chunks 89.9, 32 chunks 98.8, 64 chunks 97.0 samples/s)
        p->attn_bwd_chunks = swv2_attn_bias_chunks(Bw);
        // the weight-gradient workspace is idle until the attention backward is through (the products before it are complete, the next
        // comes after it on the same stream): the workgroups' d bias tables go there and are summed by one more launch instead of 31 K
        // atomics per workgroup -- unless the caller sums them itself for all blocks (swv2_cpb_bwd_multi): then they stay in dbias_part
        p->dbias_dest = d->dbias_part ? SWV2_DBIAS_PART : ws_bytes ? SWV2_DBIAS_WGRAD_WS : SWV2_DBIAS_ATOMICS;
    } else if (d->Lp == 176 && h <= 256) {
        // without bias at the 176-token window one workgroup (11 waves, ~90 KB of LDS) fills a CU: exactly one persistent
        // workgroup per CU (256 / heads chunks) instead of two rounds of 256 (same box: 110.4 vs 116.2 us per launch)
        p->attn_bwd_chunks = 256 / h;
    }

    auto fwd = [&](int s) { p->fwd[p->n_fwd++] = s; };
    auto bwd = [&](int s) { p->bwd[p->n_bwd++] = s; };
    const bool wide = d->DP > 64;        // wide heads (96 .. 256 columns): squared norms accumulate in rnorm, finished by swv2_qk_normalize
    if (wide) fwd(SWV2_STEP_RNORM_ZERO);
    fwd(SWV2_STEP_QKV);
    if (wide) fwd(SWV2_STEP_QK_NORMALIZE);
    if (d->bias && d->bias_pack && !d->bias_prepacked) fwd(SWV2_STEP_PACK_BIAS);
    fwd(SWV2_STEP_ATTN_FWD);
    if (p->proj_ln_fused) fwd(SWV2_STEP_PROJ_LN_FWD);
    else { fwd(SWV2_STEP_PROJ); fwd(SWV2_STEP_LN1_FWD); }
    if (p->mlp_fused) fwd(SWV2_STEP_MLP_FWD);
    else { fwd(SWV2_STEP_FC1); fwd(SWV2_STEP_FC2); fwd(SWV2_STEP_LN2_FWD); }

    const bool single = !p->wgrad_grouped;      // each weight gradient right behind the kernel that completes its operands
    if (p->mlp_fused) {
        bwd(SWV2_STEP_MLP_BWD);
        if (single) { bwd(SWV2_STEP_WGRAD_FC2); bwd(SWV2_STEP_WGRAD_FC1); }
    } else {
        bwd(SWV2_STEP_LN2_BWD); bwd(SWV2_STEP_WGRAD_FC2); bwd(SWV2_STEP_DH); bwd(SWV2_STEP_WGRAD_FC1); bwd(SWV2_STEP_DX1);
    }
    bwd(p->proj_ln_fused ? SWV2_STEP_PROJ_LN_BWD : SWV2_STEP_LN1_BWD);
    if (single) bwd(SWV2_STEP_WGRAD_PROJ);
    if (!p->proj_ln_fused) bwd(SWV2_STEP_DOH);
    bwd(SWV2_STEP_ATTN_BWD);
    if (single) bwd(SWV2_STEP_WGRAD_QKV);
    bwd(SWV2_STEP_DX);
    // d gamma / d beta of both LayerNorms: one reduction for both -- riding on the weight-gradient reduction launch when the grouped
    // products run (swv2_block_wgrad_ln), a launch of its own otherwise.  (Not deferred: each LayerNorm backward folds its own rows)
    if (p->ln_deferred && single) bwd(SWV2_STEP_LN_FOLD);
    if (p->wgrad_grouped) bwd(SWV2_STEP_WGRAD_GROUP);
    return SWV2_OK;
}

}  // namespace

extern "C" int swv2_block_step_id(int step) { return step > 0 && step < SWV2_STEP_COUNT ? STEPS[step].id : -1; }
extern "C" const char* swv2_block_step_name(int step) { return step > 0 && step < SWV2_STEP_COUNT ? STEPS[step].name : nullptr; }

// plan_block's answer plus, for a grouped launch, the kernel swv2_block_wgrad picks for it (that query reads the current device's CU count)
extern "C" int swv2_block_plan(const swv2_block_desc* d, swv2_block_plan_t* p) {
    TRY(plan_block(d, p));
    if (p->wgrad_grouped) {
        swv2_wgrad_item it[4] = {};
        wgrad_items(d, true, it);
        p->wgrad_kernel = swv2_block_wgrad_kernel(it, 0, d->wgrad_ws_bytes);
    }
    return SWV2_OK;
}

extern "C" int swv2_block_fwd(const swv2_block_desc* d, void* st) {
    SWV2_CHECK_ARG(d && d->x && d->x2 && d->qkvh && d->rowidx, "swv2_block_fwd: null descriptor field");
    swv2_block_plan_t p;
    TRY(plan_block(d, &p));
    SWV2_CHECK_ARG(d->hact || !p.need_hact_bytes, "swv2_block_fwd: the separate MLP kernels need hact (swv2_block_plan: need_hact_bytes)");
    const int BT = d->B * d->T, Bw = d->B * d->nwh * d->nww, Mw = Bw * d->Lp, C = d->C, h = d->heads, hid = d->hidden;
    for (int i = 0; i < p.n_fwd; ++i) switch (p.fwd[i]) {
    case SWV2_STEP_RNORM_ZERO:
        if (hipMemsetAsync(d->rnorm, 0, (size_t)Bw * h * 2 * d->Lp * sizeof(float), (hipStream_t)st) != hipSuccess) {
            swv2_set_error("swv2_block_fwd: hipMemsetAsync(rnorm) failed");
            return SWV2_ERR_LAUNCH;
        }
        break;
    case SWV2_STEP_QKV: {          // roll + partition gather | qkv GEMM | + bias, split heads, L2-normalise q, k
        swv2_operand a = op(SWV2_OP_F32, d->x, Mw, C, C, d->rowidx);
        swv2_epilogue e = epi(SWV2_EPI_QKV_HEADS, d->qkvh, 0, d->qkv_b_pad, nullptr, d->rnorm);
        e.p[0] = h; e.p[2] = d->Lp; e.p[3] = d->DP; e.p[4] = d->L;
        LAUNCH(SWV2_STEP_QKV, swv2_linear(&a, d->w_qkv, &e, 3 * h * d->DP, st));
    } break;
    case SWV2_STEP_QK_NORMALIZE: TRY(swv2_qk_normalize(d->qkvh, (float*)d->rnorm, Bw, h, d->Lp, d->L, d->DP, st)); break;
    // (the CPB table is packed once into the kernels' layouts; the backward reuses it)
    case SWV2_STEP_PACK_BIAS: TRY(swv2_attn_pack_bias(d->bias, h, d->L, d->bias_pack, st)); break;
    case SWV2_STEP_ATTN_FWD: {     // cosine attention core
        swv2_attn_args a = attn(d, p.attn_fwd_chunks);
        LAUNCH(SWV2_STEP_ATTN_FWD, swv2_attn_fwd(&a, st));
    } break;
    case SWV2_STEP_PROJ_LN_FWD: {  // merge heads, proj GEMM, LN1 + drop-path + residual + reverse / un-roll scatter in one kernel
        swv2_proj_ln_args m = {};
        m.oh = d->oh; m.wp = d->w_proj; m.bp = d->proj_b; m.gamma = d->n1_w; m.beta = d->n1_b; m.scale = d->dp1; m.rowidx = d->rowidx;
        m.x = d->x; m.a1 = d->a1; m.mean = d->mean1; m.rstd = d->rstd1; m.y = d->x1; m.Bw = Bw; m.Lp = d->Lp; m.heads = h; m.C = C;
        m.rows_per_sample = d->T; m.eps = 1e-5f;
        LAUNCH(SWV2_STEP_PROJ_LN_FWD, swv2_proj_ln_fwd(&m, st));
    } break;
    case SWV2_STEP_PROJ: {         // merge heads | proj GEMM
        swv2_operand a = op_heads(d->oh, Bw, h, 1, d->Lp, d->DP);
        swv2_epilogue e = epi(SWV2_EPI_BF16, d->a1, C, d->proj_b);
        LAUNCH(SWV2_STEP_PROJ, swv2_linear(&a, d->w_proj, &e, C, st));
    } break;
    case SWV2_STEP_LN1_FWD: {      // LN1 + drop-path + residual, scattered through reverse + un-roll
        swv2_ln_args l = {};
        l.a = d->a1; l.res = d->x; l.gamma = d->n1_w; l.beta = d->n1_b; l.scale = d->dp1; l.rowidx = d->rowidx; l.y = d->x1;
        l.mean = d->mean1; l.rstd = d->rstd1; l.M = Mw; l.C = C; l.res_mod = 0; l.rows_per_sample = d->T; l.eps = 1e-5f;
        LAUNCH(SWV2_STEP_LN1_FWD, swv2_ln_residual_fwd(&l, st));
    } break;
    case SWV2_STEP_MLP_FWD: {      // fc1, GELU, fc2, LN2 + drop-path + residual in one kernel (the hidden activation stays in registers)
        swv2_mlp_args m = {};
        m.x = d->x1; m.w1 = d->w_fc1; m.b1 = d->fc1_b; m.w2 = d->w_fc2; m.b2 = d->fc2_b; m.gamma = d->n2_w; m.beta = d->n2_b;
        m.scale = d->dp2; m.hpre = d->hpre; m.a2 = d->a2; m.mean = d->mean2; m.rstd = d->rstd2; m.y = d->x2;
        m.M = BT; m.C = C; m.hidden = hid; m.rows_per_sample = d->T; m.eps = 1e-5f;
        LAUNCH(SWV2_STEP_MLP_FWD, swv2_mlp_fwd(&m, st));
    } break;
    case SWV2_STEP_FC1: {          // fc1 (+ bias -> pre-activation and GELU)
        swv2_operand a = op(SWV2_OP_F32, d->x1, BT, C, C);
        swv2_epilogue e = epi(SWV2_EPI_BF16_GELU, d->hpre, hid, d->fc1_b, nullptr, (float*)d->hact);
        LAUNCH(SWV2_STEP_FC1, swv2_linear(&a, d->w_fc1, &e, hid, st));
    } break;
    case SWV2_STEP_FC2: {
        swv2_operand a = op(SWV2_OP_BF16, d->hact, BT, hid, hid);
        swv2_epilogue e = epi(SWV2_EPI_BF16, d->a2, C, d->fc2_b);
        LAUNCH(SWV2_STEP_FC2, swv2_linear(&a, d->w_fc2, &e, C, st));
    } break;
    case SWV2_STEP_LN2_FWD: {      // LN2 + drop-path + residual
        swv2_ln_args l = {};
        l.a = d->a2; l.res = d->x1; l.gamma = d->n2_w; l.beta = d->n2_b; l.scale = d->dp2; l.y = d->x2; l.mean = d->mean2;
        l.rstd = d->rstd2; l.M = BT; l.C = C; l.res_mod = 0; l.rows_per_sample = d->T; l.eps = 1e-5f;
        LAUNCH(SWV2_STEP_LN2_FWD, swv2_ln_residual_fwd(&l, st));
    } break;
    }
    return SWV2_OK;
}

extern "C" int swv2_block_bwd(const swv2_block_desc* d, void* st) {
    SWV2_CHECK_ARG(d && d->dx2 && d->dx && d->da2 && d->dh && d->dx1 && d->da1 && d->doh && d->dqkvh && d->ln_ws,
                   "swv2_block_bwd: null descriptor field");
    swv2_block_plan_t p;
    TRY(plan_block(d, &p));
    SWV2_CHECK_ARG(d->hact || !p.need_hact_bytes, "swv2_block_bwd: the separate MLP kernels need hact (swv2_block_plan: need_hact_bytes)");
    const int BT = d->B * d->T, Bw = d->B * d->nwh * d->nww, Mw = Bw * d->Lp, C = d->C, h = d->heads, hid = d->hidden;
    const int sp = d->wgrad_splits > 0 ? d->wgrad_splits : 64;
    swv2_wgrad_item it[4] = {};
    wgrad_items(d, p.mlp_fused, it);
    // deferred fold: LN2's partial rows at ln_ws, LN1's behind them, their numbers reported by the two fused kernels
    float* const ln1_ws = p.ln_deferred ? d->ln_ws + swv2_mlp_bwd_ws_floats(BT, C) : d->ln_ws;
    int n_ln1 = 0, n_ln2 = 0;
    for (int i = 0; i < p.n_bwd; ++i) switch (const int s = p.bwd[i]; s) {
    case SWV2_STEP_MLP_BWD: {      // LN2 backward, dh = (da2 W2) * GELU'(hpre), dx1 = dx2 + dh W1 in one kernel
        swv2_mlp_bwd_args m = {};
        m.dy = d->dx2; m.a2 = d->a2; m.mean = d->mean2; m.rstd = d->rstd2; m.gamma = d->n2_w; m.scale = d->dp2; m.hpre = d->hpre;
        m.w2t = d->w_fc2t; m.w1t = d->w_fc1t; m.da2 = d->da2; m.dh = d->dh; m.dx = d->dx1; m.dgamma = d->d_n2_w;
        m.dbeta = d->d_n2_b; m.ws = d->ln_ws; m.M = BT; m.C = C; m.hidden = hid; m.rows_per_sample = d->T;
        LAUNCH(SWV2_STEP_MLP_BWD, swv2_mlp_bwd_impl(&m, st, p.ln_deferred ? &n_ln2 : nullptr, p.grad_zero_in_kernel ? (float*)d->grad_zero : nullptr,
                                                    (long)(d->grad_zero_bytes / 4)));
    } break;
    case SWV2_STEP_LN2_BWD: {
        swv2_ln_args l = {};
        l.a = d->a2; l.dy = d->dx2; l.gamma = d->n2_w; l.scale = d->dp2; l.mean = d->mean2; l.rstd = d->rstd2; l.da = d->da2;
        l.dgamma = d->d_n2_w; l.dbeta = d->d_n2_b; l.ws = d->ln_ws; l.M = BT; l.C = C; l.rows_per_sample = d->T;
        LAUNCH(SWV2_STEP_LN2_BWD, swv2_ln_residual_bwd(&l, st));
    } break;
    case SWV2_STEP_WGRAD_FC2: case SWV2_STEP_WGRAD_FC1: case SWV2_STEP_WGRAD_PROJ: case SWV2_STEP_WGRAD_QKV: {
        // one product as a launch of its own (sp row slices, the block's workspace): da2^T GELU(h), dh^T x1, da1^T merge(oh), dqkv^T gather(x)
        const swv2_wgrad_item& w = it[s == SWV2_STEP_WGRAD_FC2 ? 0 : s == SWV2_STEP_WGRAD_FC1 ? 1 : s == SWV2_STEP_WGRAD_PROJ ? 2 : 3];
        LAUNCH(s, swv2_wgrad_launch(w, sp, d->wgrad_ws, d->wgrad_ws_bytes, st));
    } break;
    case SWV2_STEP_DH: {           // dh = (da2 W2) * GELU'(h)
        swv2_epilogue e = epi(SWV2_EPI_GELU_GRAD, d->dh, hid, nullptr, d->hpre);
        LAUNCH(SWV2_STEP_DH, swv2_linear(&it[0].dy, d->w_fc2t, &e, hid, st));
    } break;
    case SWV2_STEP_DX1: {          // dx1 = dx2 + dh W1
        swv2_epilogue e = epi(SWV2_EPI_F32, d->dx1, C, nullptr, d->dx2);
        LAUNCH(SWV2_STEP_DX1, swv2_linear(&it[1].dy, d->w_fc1t, &e, C, st));
    } break;
    case SWV2_STEP_PROJ_LN_BWD: {  // LN1 backward (row gather) and d(oh) = split(da1 Wp) in one kernel
        swv2_proj_ln_bwd_args m = {};
        m.dy = d->dx1; m.a1 = d->a1; m.mean = d->mean1; m.rstd = d->rstd1; m.gamma = d->n1_w; m.scale = d->dp1; m.rowidx = d->rowidx;
        m.wpt = d->w_projt; m.da1 = d->da1; m.doh = d->doh; m.dgamma = d->d_n1_w; m.dbeta = d->d_n1_b; m.ws = ln1_ws;
        m.Bw = Bw; m.Lp = d->Lp; m.heads = h; m.C = C; m.rows_per_sample = d->T;
        LAUNCH(SWV2_STEP_PROJ_LN_BWD, swv2_proj_ln_bwd_impl(&m, st, p.ln_deferred ? &n_ln1 : nullptr));
    } break;
    case SWV2_STEP_LN1_BWD: {      // gathers dx1 rows through the window table; padded rows -> 0
        swv2_ln_args l = {};
        l.a = d->a1; l.dy = d->dx1; l.gamma = d->n1_w; l.scale = d->dp1; l.rowidx = d->rowidx; l.mean = d->mean1; l.rstd = d->rstd1;
        l.da = d->da1; l.dgamma = d->d_n1_w; l.dbeta = d->d_n1_b; l.ws = d->ln_ws; l.M = Mw; l.C = C; l.rows_per_sample = d->T;
        LAUNCH(SWV2_STEP_LN1_BWD, swv2_ln_residual_bwd(&l, st));
    } break;
    case SWV2_STEP_DOH: {          // d(oh) = split(da1 Wp)
        swv2_epilogue e = epi(SWV2_EPI_HEADS, d->doh, 0);
        e.p[0] = h; e.p[2] = d->Lp; e.p[3] = d->DP; e.p[4] = d->L;
        LAUNCH(SWV2_STEP_DOH, swv2_linear(&it[2].dy, d->w_projt, &e, h * d->DP, st));
    } break;
    case SWV2_STEP_ATTN_BWD: {     // incl. the backward of the q / k normalisation
        swv2_attn_args a = attn(d, p.attn_bwd_chunks);
        a.doh = d->doh; a.rnorm = d->rnorm; a.dqkvh = d->dqkvh; a.dlogit_scale = d->d_logit_scale; a.dbias = d->d_bias;
        if (p.dbias_dest == SWV2_DBIAS_PART) { a.dbias_ws = d->dbias_part; a.dbias_ws_bytes = d->dbias_part_bytes; a.dbias_partials = 1; }
        if (p.dbias_dest == SWV2_DBIAS_WGRAD_WS) { a.dbias_ws = d->wgrad_ws; a.dbias_ws_bytes = d->wgrad_ws_bytes; }
        LAUNCH(SWV2_STEP_ATTN_BWD, swv2_attn_bwd(&a, st));
    } break;
    case SWV2_STEP_DX: {           // dx = dx1 + scatter(dqkv Wqkv)
        swv2_epilogue e = epi(SWV2_EPI_F32, d->dx, C, nullptr, d->dx1, nullptr, d->rowidx);
        LAUNCH(SWV2_STEP_DX, swv2_linear(&it[3].dy, d->w_qkvt, &e, C, st));
    } break;
    case SWV2_STEP_LN_FOLD:
        swv2_launch_ln_partials_reduce2(d->ln_ws, d->d_n2_w, d->d_n2_b, n_ln2, ln1_ws, d->d_n1_w, d->d_n1_b, n_ln1, C, (hipStream_t)st);
        break;
    case SWV2_STEP_WGRAD_GROUP: {  // the four products + (deferred) both LayerNorms' fold riding on their reduction launch
        swv2_ln_partials lnp = {{d->ln_ws, ln1_ws}, {d->d_n2_w, d->d_n1_w}, {d->d_n2_b, d->d_n1_b}, {n_ln2, n_ln1}, C};
        LAUNCH(SWV2_STEP_WGRAD_GROUP, swv2_block_wgrad_ln(it, 0, d->wgrad_ws, d->wgrad_ws_bytes, p.ln_deferred ? &lnp : nullptr, st));
    } break;
    }
    return SWV2_OK;
}
