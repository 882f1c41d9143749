// cnf_api_grad.hip — the gradient entry points of the C ABI (include/cnf.h): cnf_loss_grad_fixed / _grid / _adaptive, cnf_grad_path, cnf_integrate_*_vjp[_cond].
// In file order: who serves a call (api_grad_call: ONE resolved GradCall per call), the layouts of the gradient workspace (FusedWs, SharedWs), the
// checkpointing forward pass of the per-wave kernels (ckpt_forward), one function per implementation (grad_fused / _slab / _coop / _layered), the entries.
#include "cnf_handle.h"

using namespace cnf;

namespace {
int fail(int code, const std::string& msg) { return cnf::api_fail(code, msg); }
}  // namespace

// The configuration the fused gradient kernels are selected and packed for.  TestMode (exact trace): -tr J is the sum over
// the D unit vectors e_k of -e_k^T J e_k, i.e. the several-probe reverse sweep with K = D one-hot probes of weight 1 and no
// regularisers (the probe loop of cnf_grad2_probes.hip has no capacity limit; shapes outside the fused kernels take the
// layer-wise path).
cnf_config cnf::api_grad_cfg(const cnf_handle* h) {
    cnf_config c = h->cfg;
    if (c.mode == CNF_MODE_EXACT) {
        c.mode = CNF_MODE_HUTCH_VJP;
        c.nprobes = h->D;
        c.reg_z = c.reg_j = c.reg_aug = 0;
    }
    return c;
}

__global__ void unit_probes_kernel(float* __restrict__ eps, int D, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long DD = (long long)D * D;
    if (i >= DD * B) return;
    const int r = (int)(i % DD);
    eps[i] = (r / D) == (r % D) ? 1.f : 0.f;   // probe k = rows k D .. k D + D - 1 of the column: e_k
}

// fused reverse-sweep kernel, unless CNF_GRAD_LAYERED=1 forces the layer-wise path (tests, A/B timing)
static bool grad_is_fused(const cnf_handle* h) {
    return h->path == CNF_PATH_MFMA && grad_supported(api_grad_cfg(h)) && mfma_plan_is_per_wave(h->plan) && tuning().grad_layered == 0;
}

// the cooperative reverse sweep beats the slab kernel on the shapes that have both at every batch size: 86 -> 80 ms at 2 x 104,
// 106 -> 84 ms at 2 x 128, B = 65 536 (round 3, which set a threshold of 4096 columns for the sweep's 40 + 160 launches to
// amortise) - and, measured in round 5, 12.4 -> 7.4 ms at nvariables = 12 / 13 and 18.2 -> 8.4 ms at 14 / 15 at B = 1024 (64 ... 4000
// columns alike: the slab kernel is one wave per 16-sample tile, a latency chain; profiles/r5/r5y_mid_width_small_batches.json)
// 5 - 6 hidden tiles (nvariables = 8 ... 11, on the 8-tile instance): the sweep wins up to 8192 columns = two 16-sample super-tiles per
// CU (B = 1024: 9.0 -> 6.4 ms at nvariables = 10; 8192: 11.4 -> 8.3), the slab kernel beyond (10 240: 11.6 against 13.1 ms; 65 536:
// 47.7 against 55.1) - the auxiliary plan serves them up to 8192 columns.
static bool grad_uses_coop_aux(const cnf_handle* h, int64_t B) {
    if (!h->grad.plan_cg || !h->grad.cg_packed || B < 1) return false;
    const int sw = tuning().coop_grad_mid;   // > 1: "from sw columns on" (A/B runs, tests of the slab kernel below it)
    if (sw > 1) return B >= sw;
    return h->cfg.widths[1] > 96 || B <= 8192;
}

// Which implementation serves a call on the handle itself, and the plan and image it runs on
static GradCall own_route(const cnf_handle* h, int64_t B, int alg, bool on_grid) {
    GradCall r{};
    r.srv = const_cast<cnf_handle*>(h); r.plan = h->plan; r.image = h->par.packed_dev;
    if (grad_is_fused(h) && (h->grad.packed || !h->par.have)) { r.path = 1; return r; }
    // slab-accumulator kernel for the mid-width two-hidden-layer nets (CNF_GRAD_LAYERED=1 skips it too)
    const bool slab = (h->grad.slab_packed || !h->par.have) && grad_slab_supported(h->cfg) && tuning().grad_layered == 0;
    // B < 0: "the batch is not known" - the auxiliary cooperative plan of a slab shape is not counted (cnf_grad_path)
    const bool fits = B < 0 || B <= coop_grad_max_columns(h->cfg, alg);
    const float lam0[3] = {0.f, 0.f, 0.f};
    if (B >= 0 && grad_uses_coop_aux(h, B) && fits && coop_grad_eligible(h->cfg, h->grad.plan_cg, lam0, on_grid)) {
        r.path = 3; r.plan = h->grad.plan_cg; r.image = h->grad.cg_packed; return r;
    }
    if (slab) { r.path = 1; r.slab = true; return r; }
    // CNF_LAYERED_LOSS_BY_SOLVE (A/B switch of the layer-wise path: loss from a separate solve) keeps the call layer-wise
    if (fits && !tuning().layered_loss_by_solve && (h->par.packed_dev || !h->par.have) && coop_grad_eligible(h->cfg, h->plan, lam0, on_grid)) { r.path = 3; return r; }
    r.path = layered_grad_supported(h->cfg) ? 2 : 0;
    return r;
}

// The ONE place that decides which implementation serves a gradient call (the query entries, cnf_create and loss_grad_impl all ask it).
// Who serves it (cnf_handle::grad_twin): the handle itself; for JVP mode without the Jacobian regulariser its VJP-mode
// twin when that one has a fused implementation (1 or 3) for the call; for several probes without a fused implementation of their
// own the one-probe twin, once per probe (`nloop` = K), when that one runs on the cooperative reverse sweep.
GradCall cnf::api_grad_call(const cnf_handle* h, int64_t B, int alg, bool on_grid) {
    const GradCall own = own_route(h, B, alg, on_grid);
    if (h->grad_twin) {
        if (h->cfg.mode == CNF_MODE_HUTCH_JVP) {
            const GradCall t = api_grad_call(h->grad_twin, B, alg, on_grid);
            if (t.path == 1 || t.path == 3) return t;
        } else if (own.path != 1 && own.path != 3) {
            GradCall t = own_route(h->grad_twin, B, alg, on_grid);
            // measured at K = 4, B = 32 768 (profiles/probes_wide_timing.py, profiles/r6/r6z_probes_wide_timing.json): 1.76 - 1.78 x the
            // layer-wise path on two hidden layers (the reference's default architecture); on 3 x 256 0.96 x with the recomputing sweeps
            // of round 5 and 1.22 x with the cooperative gradient's second form (345 against 420 ms) - so three hidden layers take the
            // loop where the twin's call takes that form (asked with one step: a store that does not fit HBM falls back to the older
            // sweeps inside the loop), else keep their layer-wise gradient unless CNF_PROBE_GRAD_TWIN=2 asks for the loop
            bool loop = t.path == 3 && (h->cfg.n_layers == 3 || tuning().probe_grad_twin == 2);
            if (t.path == 3 && !loop && tuning().probe_grad_twin == 1 && B > 0)
                loop = coop_grad_stage_store_tiles(t.srv->cfg, t.plan, B, alg, 1, on_grid) > 0;
            if (loop) { t.nloop = h->cfg.nprobes; return t; }
        }
    }
    return own;
}

// Can the forward instance of `f` hand the checkpoints of a solve it runs anyway to the fused per-wave gradient kernels (CNF_ADAPTIVE_CKPT=0:
// never)?  Asked of the handle that runs that solve: the serving one on uniform steps, the caller's in cnf_loss_grad_adaptive.
static bool fwd_hands_over_ckpt(const cnf_handle* f) {
    return tuning().adaptive_ckpt != 0 && f->path == CNF_PATH_MFMA && f->plan && mfma_plan_is_per_wave(f->plan);
}

extern "C" {

int cnf_grad_path(const cnf_handle* h) {
    if (!h) return CNF_ERR_INVALID;
    return api_grad_call(h, -1, CNF_ALG_TSIT5, false).path;
}

int cnf_grad_path_for(const cnf_handle* h, int64_t B, int alg, int on_grid) {
    if (!h || B < 0 || (alg != CNF_ALG_RK4 && alg != CNF_ALG_TSIT5)) return CNF_ERR_INVALID;
    return api_grad_call(h, B, alg, on_grid != 0).path;
}

int cnf_grad_form_for(const cnf_handle* h, int64_t B, int alg, int nsteps, int on_grid) {
    if (!h || B < 0 || nsteps < 1 || (alg != CNF_ALG_RK4 && alg != CNF_ALG_TSIT5)) return CNF_ERR_INVALID;
    const GradCall c = api_grad_call(h, B, alg, on_grid != 0);
    if (c.path != 3) return 0;
    return coop_grad_stage_store_tiles(c.srv->cfg, c.plan, B, alg, nsteps, on_grid != 0) > 0 ? 2 : 1;
}

}  // extern "C"

// Layout of the fused per-wave gradient's workspace (cnf_handle::grad.ws) for `steps` steps: z checkpoints (steps + 1 slots), stage
// derivatives (steps x stages slots), logp + regs (4 B), the gradient slabs, the ping-pong states of a grid's step-by-step forward
// pass, the unit probes of TestMode.  The regions as offsets into the buffer, once it holds need_floats; `zslot`: floats of one slot.
// `yimg` (asked for by the pullback with ys_bar only, behind everything else): the image of W_1[:, ycols]^T, packed per call.
struct FusedWs { size_t ckpt, ckpt_k, logp, regs, slab, states, unit, zslot, unit_floats, need_floats, yimg; };
static FusedWs fused_ws(cnf_handle* h, int alg, int steps, int64_t B, bool on_grid, bool with_yimg = false) {
    FusedWs W{};
    const int nstages = alg == CNF_ALG_RK4 ? 4 : 6;
    W.zslot = (size_t)((B + 15) / 16) * 64 * (size_t)mfma_plan_zr(h->plan);
    W.ckpt_k = (size_t)(steps + 1) * W.zslot;
    W.logp = W.ckpt_k + (size_t)steps * nstages * W.zslot;
    W.regs = W.logp + (size_t)B;
    W.slab = W.regs + 3 * (size_t)B;
    W.states = W.slab + grad_slab_floats(api_grad_cfg(h), h->num_cus);
    W.unit = W.states + (on_grid ? 2 * (size_t)h->S * (size_t)B : 0);
    W.unit_floats = h->cfg.mode == CNF_MODE_EXACT ? (size_t)h->D * (size_t)h->D * (size_t)B : 0;
    W.need_floats = W.unit + W.unit_floats;
    if (with_yimg) { W.yimg = (W.need_floats + 63) / 64 * 64; W.need_floats = W.yimg + grad_yimg_floats(); }
    return W;
}

// Layout of the same workspace on the other routes: logp, regs and one augmented state ((S + 4) B floats) at its head; behind them,
// where a forward solve hands its checkpoints to the slab-accumulator kernel, z checkpoints (steps + 1 slots) and stage derivatives
// (steps x stages slots) in the layout of the forward instance, whose state rows `zr` gives (0: no checkpoints).  Offsets, as above.
struct SharedWs { size_t logp, regs, state, ckpt, ckpt_k, need_floats; };
static SharedWs shared_ws(const cnf_handle* h, int zr, int alg, int steps, int64_t B) {
    SharedWs W{};
    const int nstages = alg == CNF_ALG_RK4 ? 4 : 6;
    const size_t zslot = (size_t)((B + 15) / 16) * 64 * (size_t)zr;
    W.regs = (size_t)B;
    W.state = 4 * (size_t)B;
    W.ckpt = ((size_t)h->S + 4) * (size_t)B;
    W.ckpt_k = W.ckpt + (size_t)(steps + 1) * zslot;
    W.need_floats = W.ckpt_k + (size_t)nstages * steps * zslot;
    return W;
}

// What the adaptive solve that found the grid hands to the gradient on it: its final state for the loss terms and - `cap` > 0 - the checkpoints of
// its accepted steps (api_solve_tsit5's TsitCkpt) in the serving handle's workspace, laid out for `cap` steps with the state rows `zr` of its instance
struct PreparedCkpt { int cap; const float* u_final; int zr; };

// one gradient call as the entry points take it; tgrid_dev is filled by loss_grad_impl
struct LossGradArgs {
    const char* who; int alg, nsteps; float t0, t1; const float* tgrid;
    const float *x, *eps, *ys; int64_t B; const float* lambdas; float *grad, *grad_x, *sums4; void* stream;
    const PreparedCkpt* pc = nullptr;
    const float* tgrid_dev = nullptr;
};

// the fused kernels read the step times from device memory (uniform loads, once per step)
static int upload_tgrid(cnf_handle* h, int nsteps, const float* tgrid, hipStream_t st, const float** tgrid_dev) {
    HIP_TRY(h->grad.tgrid_dev.reserve(((size_t)nsteps + 1 + 63) / 64 * 64));
    HIP_TRY(hipMemcpyAsync(h->grad.tgrid_dev, tgrid, ((size_t)nsteps + 1) * sizeof(float), hipMemcpyHostToDevice, st));
    *tgrid_dev = h->grad.tgrid_dev;
    return CNF_OK;
}

// The checkpointing forward pass of the per-wave kernels: z_n and the stage derivatives of every step into ckpt / ckpt_k (slots of
// `zslot` floats).  It starts from the data x (the augmented state is assembled) or from a full state u0; u_final (may be null)
// receives the state at the end, logp / regs (may be null) its loss terms.  `states`: two S x B states, `zslot`: on a grid only.
struct CkptPass { const float *x, *u0; float* u_final; float *logp, *regs; float *ckpt, *ckpt_k; size_t zslot; float* states; };
static int ckpt_forward(cnf_handle* h, int alg, int nsteps, float t0, float t1, const float* tgrid, const float* eps, const float* ys,
                        int64_t B, const CkptPass& p, hipStream_t st) {
    SolveArgs a{};
    a.eps = eps; a.ys = ys; a.B = B; a.alg = alg; a.nvars = h->cfg.nvars;
    a.reg_aug = p.logp ? api_reg_aug(h) : 0;   // (no loss terms: no epilogue, as in cnf_integrate_fixed)
    if (!tgrid) {
        a.x = p.x; a.u0 = p.u0; a.u_out = p.u_final; a.nsteps = nsteps; a.t0 = t0; a.t1 = t1;
        a.logp = p.logp; a.regs = p.regs; a.ckpt = p.ckpt; a.ckpt_k = p.ckpt_k;
        HIP_TRY(mfma_solve(h->plan, h->par.packed_dev, a, st));
        return CNF_OK;
    }
    // non-uniform grid: the checkpointing forward pass is one launch of the (unchanged) solve kernel per step - the metric
    // kernel keeps its loop-invariant step size; step n writes checkpoint slots n and n + 1 and its stage derivatives
    float* ua = p.states;
    float* ub = ua + (size_t)h->S * (size_t)B;
    const int nstages = alg == CNF_ALG_RK4 ? 4 : 6;
    if (p.x) HIP_TRY(assemble_u0(p.x, h->cfg.nvars, h->S, B, ua, st));
    const float* from = p.x ? ua : p.u0;
    a.nsteps = 1;
    for (int n = 0; n < nsteps; ++n) {
        float* to = (n == nsteps - 1 && p.u_final) ? p.u_final : (from == ua ? ub : ua);
        a.u0 = from; a.u_out = to; a.t0 = tgrid[n]; a.t1 = tgrid[n + 1];
        a.ckpt = p.ckpt + (size_t)n * p.zslot; a.ckpt_k = p.ckpt_k + (size_t)n * nstages * p.zslot;
        if (n == nsteps - 1) { a.logp = p.logp; a.regs = p.regs; }
        HIP_TRY(mfma_solve(h->plan, h->par.packed_dev, a, st));
        from = to;
    }
    return CNF_OK;
}

// the weights of the live regularisers (api_grad_cfg: the exact-trace dynamics carry none, icnf.jl:297-339)
struct Lam { float v[3]; };
static Lam live_lambdas(const cnf_handle* h, const float* lambdas) {
    const cnf_config gc = api_grad_cfg(h);
    return Lam{{gc.reg_z ? lambdas[0] : 0.f, gc.reg_j ? lambdas[1] : 0.f, api_reg_aug(h) ? lambdas[2] : 0.f}};
}

// logp / regs from the regular solve on whichever family serves the handle, for the implementations whose sweep does not yield them
// (`u`: scratch for one augmented state)
static int loss_by_solve(cnf_handle* h, const LossGradArgs& a, float* logp, float* regs, float* u, hipStream_t st) {
    if (!a.tgrid) return cnf_inference_fixed(h, a.alg, a.nsteps, a.t0, a.t1, a.x, a.eps, a.ys, a.B, logp, regs, nullptr, a.stream);
    // the adaptive solve that found the grid has the state at t1: its loss terms, no second solve over the grid
    const float* u1 = a.pc ? a.pc->u_final : nullptr;
    if (!u1) {   // the loss of the same discrete solve: augmented state advanced over the grid, then the epilogue
        HIP_TRY(assemble_u0(a.x, h->cfg.nvars, h->S, a.B, u, st));
        const int rc = api_integrate_grid(h, a.alg, a.nsteps, a.tgrid, u, a.eps, a.ys, a.B, st);
        if (rc) return rc;
        u1 = u;
    }
    HIP_TRY(epilogue(u1, h->cfg.nvars, h->D, api_reg_aug(h), a.B, logp, regs, st));
    return CNF_OK;
}

// path 1, register accumulators (cnf_grad2.hip, cnf_grad2_probes.hip): the checkpointing forward pass, which also yields the loss
// terms, then ONE launch for the whole reverse sweep
static int grad_fused(cnf_handle* h, const LossGradArgs& a, hipStream_t st) {
    HIP_TRY(api_num_cus(h));
    const cnf_config gc = api_grad_cfg(h);
    const bool exact = h->cfg.mode == CNF_MODE_EXACT;
    // (checkpoints an adaptive solve has written sit in arrays laid out for pc->cap steps, of which the first nsteps are filled)
    // (a final state without checkpoints serves the other implementations' loss terms only)
    const PreparedCkpt* pc = (a.pc && a.pc->cap > 0) ? a.pc : nullptr;
    const FusedWs W = fused_ws(h, a.alg, pc ? pc->cap : a.nsteps, a.B, a.tgrid != nullptr);
    if (pc && W.need_floats > h->grad.ws.capacity()) return fail(CNF_ERR_INVALID, std::string(a.who) + ": prepared checkpoints without their workspace");
    HIP_TRY(h->grad.ws.reserve(W.need_floats));
    float* ws = h->grad.ws;
    if (pc) {
        // the solve that found the grid has left z_n and the stage derivatives of its accepted steps in ckpt / ckpt_k: no forward
        // pass; the loss terms are those of its final state
        HIP_TRY(epilogue(pc->u_final, h->cfg.nvars, h->D, api_reg_aug(h), a.B, ws + W.logp, ws + W.regs, st));
    } else {
        const CkptPass p{a.x, nullptr, nullptr, ws + W.logp, ws + W.regs, ws + W.ckpt, ws + W.ckpt_k, W.zslot, ws + W.states};
        const int rc = ckpt_forward(h, a.alg, a.nsteps, a.t0, a.t1, a.tgrid, a.eps, a.ys, a.B, p, st);
        if (rc) return rc;
    }
    if (a.sums4) {
        HIP_TRY(api_loss_partial(h));
        HIP_TRY(loss_sums(ws + W.logp, ws + W.regs, a.B, h->loss_partial, a.sums4, st));
    }
    const Lam lam = live_lambdas(h, a.lambdas);
    const float* probes = a.eps;
    if (exact) {
        hipLaunchKernelGGL(unit_probes_kernel, dim3((unsigned)((W.unit_floats + 255) / 256)), dim3(256), 0, st, ws + W.unit, h->D, (long long)a.B);
        HIP_TRY(hipGetLastError());
        probes = ws + W.unit;
    }
    HIP_TRY(grad_launch(gc, h->grad.packed, ws + W.ckpt, ws + W.ckpt_k, mfma_plan_zr(h->plan), probes, a.ys, h->par.w_off.data(), h->par.b_off.data(), a.alg,
                        a.nsteps, a.t0, a.t1, a.tgrid_dev, exact ? 1.f : 0.f, a.B, lam.v, ws + W.slab, a.grad, a.grad_x, h->num_cus, st));
    return CNF_OK;
}

// path 1, slab accumulators - two-hidden-layer nets of 4..7 hidden tiles: tile-fused reverse sweep with slab accumulators
// (cnf_grad_slab.hip).  Its forward sweep is inside the kernel, unless a forward solve that runs anyway has left checkpoints.
static int grad_slab(cnf_handle* h, const LossGradArgs& a, hipStream_t st) {
    // checkpoints the adaptive solve that found the grid has written (for pc->cap steps, in its forward instance's layout)
    const bool pre = a.pc && a.pc->cap > 0 && a.tgrid;
    // slab-accumulator kernel on uniform steps: ONE forward solve serves both the loss terms and - through its checkpoints, in the
    // forward instance's layout, kept behind the loss workspace - the kernel, which then runs no forward sweep of its own
    const bool shared = !a.tgrid && a.sums4 && fwd_hands_over_ckpt(h) && h->par.packed_dev;
    const int zr = pre ? a.pc->zr : (shared ? mfma_plan_zr(h->plan) : 0);
    const SharedWs SW = shared_ws(h, zr, a.alg, pre ? a.pc->cap : a.nsteps, a.B);
    if (a.sums4) HIP_TRY(h->grad.ws.reserve(SW.need_floats));   // (`pre`: the solve that wrote them has made the buffer hold them)
    float* ws = h->grad.ws;
    if (a.sums4) {
        const CkptPass p{a.x, nullptr, nullptr, ws + SW.logp, ws + SW.regs, ws + SW.ckpt, ws + SW.ckpt_k, 0, nullptr};
        const int rc = shared ? ckpt_forward(h, a.alg, a.nsteps, a.t0, a.t1, nullptr, a.eps, a.ys, a.B, p, st)
                              : loss_by_solve(h, a, ws + SW.logp, ws + SW.regs, ws + SW.state, st);   // (the kernel itself yields no loss terms)
        if (rc) return rc;
        HIP_TRY(api_loss_partial(h));
        HIP_TRY(loss_sums(ws + SW.logp, ws + SW.regs, a.B, h->loss_partial, a.sums4, st));
    }
    const Lam lam = live_lambdas(h, a.lambdas);
    HIP_TRY(api_num_cus(h));
    HIP_TRY(h->grad.slab_ws.reserve(grad_slab_ws_floats(h->cfg, a.alg, a.nsteps, a.B, h->num_cus)));
    HIP_TRY(grad_slab_launch(h->cfg, h->grad.slab_packed, a.x, a.eps, a.ys, h->par.w_off.data(), h->par.b_off.data(), a.alg, a.nsteps, a.t0, a.t1,
                             a.tgrid_dev, a.B, lam.v, h->grad.slab_ws, a.grad, a.grad_x, h->num_cus, st, zr ? ws + SW.ckpt : nullptr,
                             zr ? ws + SW.ckpt_k : nullptr, zr));
    return CNF_OK;
}

// path 3 - wide hidden layers on the cooperative kernels: checkpointing forward solve (which also yields the loss terms),
// one reverse-sweep launch per step, deferred weight-cotangent products (cnf_coop_grad.hip)
static int grad_coop(cnf_handle* h, const GradCall& c, const LossGradArgs& a, hipStream_t st) {
    const SharedWs SW = shared_ws(h, 0, a.alg, a.nsteps, a.B);
    if (a.sums4) {
        HIP_TRY(h->grad.ws.reserve(SW.need_floats));
        HIP_TRY(api_loss_partial(h));
    }
    float* ws = h->grad.ws;
    const Lam lam = live_lambdas(h, a.lambdas);
    if (!c.image) return fail(CNF_ERR_NO_PARAMS, std::string(a.who) + ": cnf_set_params has not been called");
    std::string msg;
    hipError_t e = coop_grad(&h->grad.layered, h->cfg, c.plan, c.image, h->par.w_off.data(), h->par.b_off.data(), a.x, a.eps, a.ys, a.alg, a.nsteps,
                             a.t0, a.t1, a.tgrid, a.tgrid_dev, a.B, lam.v, a.grad, a.grad_x, a.sums4 ? ws + SW.logp : nullptr,
                             a.sums4 ? ws + SW.regs : nullptr, st, &msg);
    if (e != hipSuccess) return fail(CNF_ERR_HIP, std::string(a.who) + ": " + msg);
    if (a.sums4) HIP_TRY(loss_sums(ws + SW.logp, ws + SW.regs, a.B, h->loss_partial, a.sums4, st));
    return CNF_OK;
}

// path 2 - the layer-wise reverse sweep (cnf_layered.hip) accumulates the loss terms of the solve it differentiates, unless
// CNF_LAYERED_LOSS_BY_SOLVE asks for a separate solve
static int grad_layered(cnf_handle* h, const LossGradArgs& a, hipStream_t st) {
    const bool in_sweep = a.sums4 && !tuning().layered_loss_by_solve;
    const SharedWs SW = shared_ws(h, 0, a.alg, a.nsteps, a.B);
    if (a.sums4) HIP_TRY(h->grad.ws.reserve(SW.need_floats));
    float* ws = h->grad.ws;
    if (a.sums4 && !in_sweep) {
        const int rc = loss_by_solve(h, a, ws + SW.logp, ws + SW.regs, ws + SW.state, st);
        if (rc) return rc;
    }
    if (a.sums4) HIP_TRY(api_loss_partial(h));
    if (a.sums4 && !in_sweep) HIP_TRY(loss_sums(ws + SW.logp, ws + SW.regs, a.B, h->loss_partial, a.sums4, st));
    const Lam lam = live_lambdas(h, a.lambdas);
    std::string msg;
    hipError_t e = layered_grad(&h->grad.layered, h->cfg, h->par.P_dev, h->par.w_off.data(), h->par.b_off.data(), a.x, a.eps, a.ys, a.alg, a.nsteps,
                                a.t0, a.t1, a.tgrid, a.B, lam.v, a.grad, a.grad_x, st, &msg, in_sweep ? ws + SW.logp : nullptr,
                                in_sweep ? ws + SW.regs : nullptr);
    if (e == hipErrorNotSupported) return fail(CNF_ERR_UNSUPPORTED, std::string(a.who) + ": " + msg);
    if (e != hipSuccess) return fail(CNF_ERR_HIP, std::string(a.who) + ": " + msg);
    if (in_sweep) HIP_TRY(loss_sums(ws + SW.logp, ws + SW.regs, a.B, h->loss_partial, a.sums4, st));
    return CNF_OK;
}

static int loss_grad_impl(cnf_handle* h, LossGradArgs a, const GradCall* resolved = nullptr);

// rows p D .. p D + D - 1 of every column of the (K D) x B probe array: probe p as a D x B array
__global__ void probe_slice_kernel(const float* __restrict__ eps, int K, int D, int p, long long B, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)D * B) return;
    const long long b = i / D;
    out[i] = eps[b * (long long)K * D + (long long)p * D + (i - b * D)];
}

// acc = first ? w v : acc + w v
__global__ void probe_accum_kernel(float* __restrict__ acc, const float* __restrict__ v, float w, int first, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[i] = first ? w * v[i] : fmaf(w, v[i], acc[i]);
}

// Several probes through the one-probe handle `one` (cnf_handle::grad_twin): loss sums and gradients of the K one-probe calls,
// averaged in probe order.  Every call is a whole forward solve + reverse sweep of the cooperative path.
static int loss_grad_probe_loop(cnf_handle* h, cnf_handle* one, int K, const LossGradArgs& a) {
    const int64_t B = a.B;
    if ((B > 0 && (!a.x || !a.eps)) || !a.grad || !a.lambdas) return fail(CNF_ERR_INVALID, std::string(a.who) + ": null x/eps/grad/lambdas");
    DeviceGuard g(h->cfg.device_id);
    hipStream_t st = (hipStream_t)a.stream;
    const size_t D = (size_t)h->D, n = h->par.n, nx = a.grad_x ? (size_t)B * (size_t)h->cfg.nvars : 0;
    const size_t need = D * (size_t)B + n + nx + 4 + 16;
    HIP_TRY(h->grad.probe_ws.reserve(need));
    float* eps_p = h->grad.probe_ws;
    float* grad_p = eps_p + (D * (size_t)B + 3) / 4 * 4;
    float* gx_p = a.grad_x ? grad_p + (n + 3) / 4 * 4 : nullptr;
    float* sums_p = grad_p + (n + 3) / 4 * 4 + (nx + 3) / 4 * 4;
    const float w = 1.f / (float)K;
    auto accum = [&](float* acc, const float* v, size_t cnt, int first) -> hipError_t {
        if (!cnt) return hipSuccess;
        hipLaunchKernelGGL(probe_accum_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, acc, v, w, first, (long long)cnt);
        return hipGetLastError();
    };
    if (B == 0) return loss_grad_impl(one, a);
    LossGradArgs a1 = a;   // one probe's call
    a1.eps = eps_p; a1.grad = grad_p; a1.grad_x = gx_p; a1.sums4 = a.sums4 ? sums_p : nullptr;
    for (int p = 0; p < K; ++p) {
        const long long cnt = (long long)D * B;
        hipLaunchKernelGGL(probe_slice_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, a.eps, K, (int)D, p, (long long)B, eps_p);
        HIP_TRY(hipGetLastError());
        const int rc = loss_grad_impl(one, a1);
        if (rc) return rc;
        HIP_TRY(accum(a.grad, grad_p, n, p == 0));
        if (a.grad_x) HIP_TRY(accum(a.grad_x, gx_p, nx, p == 0));
        if (a.sums4) HIP_TRY(accum(a.sums4, sums_p, 4, p == 0));
    }
    return CNF_OK;
}

// loss sums + gradient on a uniform grid (tgrid == nullptr: nsteps steps from t0 to t1) or on the caller's non-uniform
// grid (tgrid: host, nsteps + 1 times; t0 / t1 ignored).  The same implementations serve both.  `resolved`: the call as
// cnf_loss_grad_adaptive has resolved it already (an unknown alg has no route: it is reported behind nsteps)
static int loss_grad_impl(cnf_handle* h, LossGradArgs a, const GradCall* resolved) {
    int rc = api_check_call(h, a.eps, a.ys, a.B, a.who);
    if (rc) return rc;
    const bool known = a.alg == CNF_ALG_RK4 || a.alg == CNF_ALG_TSIT5;
    const GradCall c = resolved ? *resolved : (known ? api_grad_call(h, a.B, a.alg, a.tgrid != nullptr) : GradCall{});
    if (c.nloop > 1) return loss_grad_probe_loop(h, c.srv, c.nloop, a);
    if (c.srv && c.srv != h) {   // a twin serves the call: from here on it is a call on the twin
        h = c.srv;
        rc = api_check_call(h, a.eps, a.ys, a.B, a.who);
        if (rc) return rc;
    }
    const std::string w(a.who);
    if (a.nsteps < 1) return fail(CNF_ERR_INVALID, w + ": nsteps >= 1 required");
    if (a.alg != CNF_ALG_RK4 && a.alg != CNF_ALG_TSIT5) return fail(CNF_ERR_INVALID, w + ": unknown alg");
    if ((a.B > 0 && !a.x) || !a.grad || !a.lambdas) return fail(CNF_ERR_INVALID, w + ": null x/grad/lambdas");
    if (c.path == 0) return fail(CNF_ERR_UNSUPPORTED, w + ": no gradient path for this configuration");
    DeviceGuard g(h->cfg.device_id);
    hipStream_t st = (hipStream_t)a.stream;
    HIP_TRY(zero_async(a.grad, h->par.n * sizeof(float), st));
    if (a.B == 0) {
        if (a.sums4) HIP_TRY(zero_async(a.sums4, 4 * sizeof(float), st));
        return CNF_OK;
    }
    if (a.tgrid) {
        a.t0 = a.tgrid[0]; a.t1 = a.tgrid[a.nsteps];
        rc = upload_tgrid(h, a.nsteps, a.tgrid, st, &a.tgrid_dev);
        if (rc) return rc;
    }
    if (c.path == 3) return grad_coop(h, c, a, st);
    if (c.path == 2) return grad_layered(h, a, st);
    return c.slab ? grad_slab(h, a, st) : grad_fused(h, a, st);
}

extern "C" {

int cnf_loss_grad_fixed(cnf_handle* h, int alg, int nsteps, float t0, float t1, const float* x,
                        const float* eps, const float* ys, int64_t B, const float* lambdas,
                        float* grad, float* grad_x, float* sums4, void* stream) {
    return loss_grad_impl(h, {"cnf_loss_grad_fixed", alg, nsteps, t0, t1, nullptr, x, eps, ys, B, lambdas, grad, grad_x, sums4, stream});
}

int cnf_loss_grad_grid(cnf_handle* h, int alg, int nsteps, const float* tgrid, const float* x, const float* eps,
                       const float* ys, int64_t B, const float* lambdas, float* grad, float* grad_x, float* sums4,
                       void* stream) {
    if (nsteps < 1 || !tgrid) return fail(CNF_ERR_INVALID, "cnf_loss_grad_grid: nsteps >= 1 and a grid of nsteps + 1 times required");
    return loss_grad_impl(h, {"cnf_loss_grad_grid", alg, nsteps, 0.f, 0.f, tgrid, x, eps, ys, B, lambdas, grad, grad_x, sums4, stream});
}

int cnf_loss_grad_adaptive(cnf_handle* h, float t0, float t1, const float* x, const float* eps, const float* ys, int64_t B,
                           float abstol, float reltol, float dt_init, int maxiters, const float* lambdas, float* grad,
                           float* grad_x, float* sums4, cnf_solve_stats* stats, float* tgrid_out, int32_t grid_cap,
                           void* stream) {
    if (stats) *stats = cnf_solve_stats{};
    int rc = api_check_call(h, eps, ys, B, "cnf_loss_grad_adaptive");
    if (rc) return rc;
    if ((B > 0 && !x) || !grad || !lambdas) return fail(CNF_ERR_INVALID, "cnf_loss_grad_adaptive: null x/grad/lambdas");
    if (t0 == t1) return fail(CNF_ERR_INVALID, "cnf_loss_grad_adaptive: empty time span");
    LossGradArgs a{"cnf_loss_grad_adaptive", CNF_ALG_TSIT5, 1, t0, t1, nullptr, x, eps, ys, B, lambdas, grad, grad_x, sums4, stream};
    if (B == 0) return loss_grad_impl(h, a);   // nothing to step over: the fixed entry zeroes grad / sums4
    std::vector<float> grid;
    PreparedCkpt pc{};
    // (c.srv: the handle whose gradient implementation serves the call - h itself, or its VJP twin for a JVP-mode handle: the solve
    // runs on h either way, and z_n / the stage derivatives do not depend on the trace engine)
    const GradCall c = api_grad_call(h, B, CNF_ALG_TSIT5, true);
    {
        DeviceGuard g(h->cfg.device_id);
        rc = api_ensure_adaptive_buf(h, B);
        if (rc) return rc;
        const size_t slot = (size_t)h->S * (size_t)h->adp.B;
        float* u = h->adp.buf + 4 * slot;
        // Where the gradient on the frozen grid is the fused per-wave sweep of this very handle, the solve that finds the grid also
        // writes the sweep's checkpoints (z_n and the stage derivatives of every accepted step: the one-launch kernel has them in
        // registers; beyond its capacity the library's host loop lets every fused attempt fill the slots of its step) - the gradient
        // then needs no forward pass of its own.  Up to kAdaptiveCkptSteps steps; a longer solve or CNF_ADAPTIVE_CKPT=0 take the
        // step-by-step forward pass of ckpt_forward.
        const int kAdaptiveCkptSteps = B <= 32768 ? 32 : 16;   // (7 slots of tiles x 64 x ZR floats a step: 225 MB at 32 768 samples, D <= 8)
        const bool eligible = c.nloop == 1 && c.path == 1 && fwd_hands_over_ckpt(h);
        TsitCkpt ck{};
        if (eligible && !c.slab && mfma_plan_zr(h->plan) == mfma_plan_zr(c.srv->plan)) {
            HIP_TRY(api_num_cus(c.srv));
            const FusedWs W = fused_ws(c.srv, CNF_ALG_TSIT5, kAdaptiveCkptSteps, B, true);
            HIP_TRY(c.srv->grad.ws.reserve(W.need_floats));
            ck.ckpt = c.srv->grad.ws + W.ckpt; ck.ckpt_k = c.srv->grad.ws + W.ckpt_k; ck.cap = kAdaptiveCkptSteps;
        } else if (eligible && c.slab) {
            // slab-accumulator gradient (its forward sweep is inside the kernel): the arrays sit behind the loss workspace,
            // in the forward instance's layout, which the kernel reads with that stride
            const SharedWs SW = shared_ws(c.srv, mfma_plan_zr(h->plan), CNF_ALG_TSIT5, kAdaptiveCkptSteps, B);
            HIP_TRY(c.srv->grad.ws.reserve(SW.need_floats));
            ck.ckpt = c.srv->grad.ws + SW.ckpt; ck.ckpt_k = c.srv->grad.ws + SW.ckpt_k; ck.cap = kAdaptiveCkptSteps;
        }
        HIP_TRY(assemble_u0(x, h->cfg.nvars, h->S, B, u, (hipStream_t)stream));
        std::vector<double> steps;
        rc = api_solve_tsit5(h, t0, t1, u, eps, ys, B, abstol, reltol, dt_init, maxiters, u + slot, stats, &steps, stream, &ck);
        if (rc) return rc;
        double t = t0;
        grid.push_back(t0);
        for (double d : steps) { t += d; grid.push_back((float)t); }
        grid.back() = t1;
        if (ck.ok && (int)steps.size() <= ck.cap) { pc.cap = ck.cap; pc.zr = mfma_plan_zr(h->plan); }
        // the state at t1: the loss terms of every implementation (a route without checkpoints still takes it; the probe loop does not)
        if (tuning().adaptive_ckpt != 0 && c.nloop == 1) { pc.u_final = u + slot; a.pc = &pc; }
    }
    if (tgrid_out)
        for (size_t i = 0; i < grid.size() && (int64_t)i < grid_cap; ++i) tgrid_out[i] = grid[i];
    a.nsteps = (int)grid.size() - 1; a.t0 = a.t1 = 0.f; a.tgrid = grid.data();
    return loss_grad_impl(h, a, &c);
}

}  // extern "C"

// ---- the pullback of base_sol (cnf_integrate_fixed_vjp / cnf_integrate_grid_vjp) ------------------------------------------------------
// The reverse sweeps above with the terminal costate and the cotangents of the dlogp / E / n rows taken from the caller (u1_bar)
// instead of from z_N and the three lambdas.  Two implementations: the fused per-wave sweep in its cotangent form (cnf_grad2_cot.hip)
// for the one-probe VJP shapes of cnf_grad.hip's table, the layer-wise sweep (cnf_layered.hip) for every other Dense chain - JVP mode,
// several probes, the exact trace, the slab and cooperative shapes (their kernels have no cotangent form).  Nothing is kept in the
// handle between calls beyond workspace capacity.
// ys_bar (cnf_integrate_*_vjp_cond; null: the call is bit for bit the one without it): the cotangent of the conditions, on the same
// routes - path 1 on the kernel of cnf_grad2_coty.hip, path 2 with one more accumulation per stage and one product per call.
static int vjp_route(const cnf_handle* h) {
    const cnf_config& c = h->cfg;
    if (grad_is_fused(h) && (h->grad.packed || !h->par.have) && c.mode == CNF_MODE_HUTCH_VJP && c.nprobes == 1) return 1;
    return (layered_grad_supported(c) && layered_supports(c)) ? 2 : 0;
}

static int integrate_vjp_impl(cnf_handle* h, const char* who, int alg, int nsteps, float t0, float t1, const float* tgrid, const float* u0,
                              const float* eps, const float* ys, int64_t B, const float* u1_bar, float* grad, float* u0_bar, float* u1,
                              void* stream, float* ys_bar = nullptr) {
    int rc = api_check_call(h, eps, ys, B, who);
    if (rc) return rc;
    const std::string w(who);
    if (nsteps < 1) return fail(CNF_ERR_INVALID, w + ": nsteps >= 1 required");
    if (alg != CNF_ALG_RK4 && alg != CNF_ALG_TSIT5) return fail(CNF_ERR_INVALID, w + ": unknown alg");
    if ((B > 0 && (!u0 || !u1_bar)) || !grad) return fail(CNF_ERR_INVALID, w + ": null u0/u1_bar/grad");
    if (B > 0 && ((u0_bar && (u0_bar == u0 || u0_bar == u1_bar || u0_bar == u1)) || (u1 && (u1 == u0 || u1 == u1_bar))))
        return fail(CNF_ERR_INVALID, w + ": u0_bar / u1 may not alias u0, u1_bar or each other");
    if (ys_bar && h->cfg.ncond == 0) return fail(CNF_ERR_INVALID, w + ": ys_bar given, but the handle has no conditions");
    if (ys_bar && B > 0 && (ys_bar == ys || ys_bar == u0 || ys_bar == u1_bar || ys_bar == u0_bar || ys_bar == u1))
        return fail(CNF_ERR_INVALID, w + ": ys_bar may not alias ys, u0, u1_bar, u0_bar or u1");
    const int path = vjp_route(h);
    if (path == 0) return fail(CNF_ERR_UNSUPPORTED, w + ": no pullback for this configuration (a layer wider than the product kernels cover)");
    DeviceGuard g(h->cfg.device_id);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(zero_async(grad, h->par.n * sizeof(float), st));
    if (B == 0) return CNF_OK;
    const bool hutch = h->cfg.mode != CNF_MODE_EXACT;   // the exact-trace dynamics carry no regularisers: their rows are identically zero
    const float sw[3] = {hutch && h->cfg.reg_z ? 1.f : 0.f, hutch && h->cfg.reg_j ? 1.f : 0.f, 0.f};
    if (tgrid) { t0 = tgrid[0]; t1 = tgrid[nsteps]; }
    if (path == 2) {
        std::string msg;
        const LayeredCot cot{u0, u1_bar, u0_bar, u1, ys_bar};
        hipError_t e = layered_grad(&h->grad.layered, h->cfg, h->par.P_dev, h->par.w_off.data(), h->par.b_off.data(), nullptr, eps, ys, alg, nsteps,
                                    t0, t1, tgrid, B, sw, grad, nullptr, st, &msg, nullptr, nullptr, &cot);
        if (e == hipErrorNotSupported) return fail(CNF_ERR_UNSUPPORTED, w + ": " + msg);
        if (e != hipSuccess) return fail(CNF_ERR_HIP, w + ": " + msg);
        return CNF_OK;
    }
    const float* tgrid_dev = nullptr;
    if (tgrid) {
        rc = upload_tgrid(h, nsteps, tgrid, st, &tgrid_dev);
        if (rc) return rc;
    }
    HIP_TRY(api_num_cus(h));
    const FusedWs W = fused_ws(h, alg, nsteps, B, tgrid != nullptr, ys_bar != nullptr);
    HIP_TRY(h->grad.ws.reserve(W.need_floats));
    float* ws = h->grad.ws;
    // the checkpointing forward solve from the caller's full state
    const CkptPass p{nullptr, u0, u1, nullptr, nullptr, ws + W.ckpt, ws + W.ckpt_k, W.zslot, ws + W.states};
    rc = ckpt_forward(h, alg, nsteps, t0, t1, tgrid, eps, ys, B, p, st);
    if (rc) return rc;
    HIP_TRY(grad_launch(api_grad_cfg(h), h->grad.packed, ws + W.ckpt, ws + W.ckpt_k, mfma_plan_zr(h->plan), eps, ys, h->par.w_off.data(), h->par.b_off.data(), alg,
                        nsteps, t0, t1, tgrid_dev, 0.f, B, sw, ws + W.slab, grad, nullptr, h->num_cus, st, u1_bar, u0_bar, ys_bar,
                        ys_bar ? (const float*)h->par.P_dev : nullptr, ys_bar ? ws + W.yimg : nullptr));
    return CNF_OK;
}

extern "C" {

int cnf_integrate_fixed_vjp(cnf_handle* h, int alg, int nsteps, float t0, float t1, const float* u0, const float* eps, const float* ys,
                            int64_t B, const float* u1_bar, float* grad, float* u0_bar, float* u1, void* stream) {
    return integrate_vjp_impl(h, "cnf_integrate_fixed_vjp", alg, nsteps, t0, t1, nullptr, u0, eps, ys, B, u1_bar, grad, u0_bar, u1, stream);
}

int cnf_integrate_grid_vjp(cnf_handle* h, int alg, int nsteps, const float* tgrid, const float* u0, const float* eps, const float* ys,
                           int64_t B, const float* u1_bar, float* grad, float* u0_bar, float* u1, void* stream) {
    if (nsteps < 1 || !tgrid) return fail(CNF_ERR_INVALID, "cnf_integrate_grid_vjp: nsteps >= 1 and a grid of nsteps + 1 times required");
    return integrate_vjp_impl(h, "cnf_integrate_grid_vjp", alg, nsteps, 0.f, 0.f, tgrid, u0, eps, ys, B, u1_bar, grad, u0_bar, u1, stream);
}

int cnf_integrate_fixed_vjp_cond(cnf_handle* h, int alg, int nsteps, float t0, float t1, const float* u0, const float* eps, const float* ys,
                                 int64_t B, const float* u1_bar, float* grad, float* u0_bar, float* ys_bar, float* u1, void* stream) {
    return integrate_vjp_impl(h, "cnf_integrate_fixed_vjp_cond", alg, nsteps, t0, t1, nullptr, u0, eps, ys, B, u1_bar, grad, u0_bar, u1, stream, ys_bar);
}

int cnf_integrate_grid_vjp_cond(cnf_handle* h, int alg, int nsteps, const float* tgrid, const float* u0, const float* eps, const float* ys,
                                int64_t B, const float* u1_bar, float* grad, float* u0_bar, float* ys_bar, float* u1, void* stream) {
    if (nsteps < 1 || !tgrid) return fail(CNF_ERR_INVALID, "cnf_integrate_grid_vjp_cond: nsteps >= 1 and a grid of nsteps + 1 times required");
    return integrate_vjp_impl(h, "cnf_integrate_grid_vjp_cond", alg, nsteps, 0.f, 0.f, tgrid, u0, eps, ys, B, u1_bar, grad, u0_bar, u1, stream, ys_bar);
}

int cnf_vjp_path_for(const cnf_handle* h, int64_t B, int alg, int on_grid) {
    (void)on_grid;
    if (!h || B < 0 || (alg != CNF_ALG_RK4 && alg != CNF_ALG_TSIT5)) return CNF_ERR_INVALID;
    return vjp_route(h);
}

}  // extern "C"
