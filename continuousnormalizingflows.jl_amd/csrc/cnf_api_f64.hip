// cnf_api_f64.hip — the double-precision entries of the C ABI (include/cnf.h: cnf_f64_supported, cnf_set_params_f64,
// cnf_aug_f_f64, cnf_integrate_fixed_f64, cnf_inference_fixed_f64).  Host side only: validation, the second parameter binding
// of the handle (cnf_handle::f64) and the launch of the one kernel of cnf_f64.hip.  Stream-ordered; nothing synchronises
// except the copy of a HOST parameter vector, as in cnf_set_params.
#include "cnf_f64.h"
#include "cnf_handle.h"

using namespace cnf;

namespace {

int fail(int code, const std::string& msg) { return cnf::api_fail(code, msg); }

// why the handle's flow cannot run in double ("" if it can), derived from the configuration alone, for a call that keeps `ns`
// stage derivatives: 6 = under every solver (cnf_f64_supported), 4 an RK4 solve, 1 a dynamics call.  *net is laid out for ns.
std::string f64_refusal(const cnf_handle* h, F64Net* net, int ns) {
    const cnf_config& c = h->cfg;
    if (c.mode == CNF_MODE_HUTCH_JVP)
        return "the double-precision path computes the trace through the pullback (CNF_MODE_HUTCH_VJP, CNF_MODE_EXACT); "
               "CNF_MODE_HUTCH_JVP runs in Float32 only";
    f64_layout(c, net, ns);
    if (net->image >= (size_t)1 << 31) return "the operand image exceeds 2^31 doubles";
    if (f64_waves(*net) < 1) {
        char buf[320];
        std::snprintf(buf, sizeof buf,
                      "one wave needs %d LDS rows of 128 bytes = %lld bytes (pad4(n_in) + sum_l pad16(out_l) + 2 max pad16(width) "
                      "+ (ns + 1) (D + 3) + K D rows, ns = %d stage derivatives); the limit is %d bytes (%d rows)",
                      net->rows, 128LL * net->rows, ns, kF64LdsBytes, kF64LdsBytes / 128);
        return buf;
    }
    return "";
}

int check_call(cnf_handle* h, F64Net* net, int ns, const double* eps, const double* ys, int64_t B, const char* who) {
    if (!h) return fail(CNF_ERR_INVALID, std::string(who) + ": null handle");
    const std::string why = f64_refusal(h, net, ns);
    if (!why.empty()) return fail(CNF_ERR_UNSUPPORTED, std::string(who) + ": " + why);
    if (!h->f64.have) return fail(CNF_ERR_NO_PARAMS, std::string(who) + ": cnf_set_params_f64 not called");
    if (B < 0) return fail(CNF_ERR_INVALID, std::string(who) + ": negative batch");
    if (h->cfg.mode != CNF_MODE_EXACT && !eps && B > 0)
        return fail(CNF_ERR_INVALID, std::string(who) + ": eps is required in Hutchinson modes");
    if (h->cfg.ncond > 0 && !ys && B > 0) return fail(CNF_ERR_INVALID, std::string(who) + ": ys is required when ncond > 0");
    return CNF_OK;
}

int check_solver(int alg, int nsteps, double t0, double t1, const char* who) {
    if (nsteps < 1) return fail(CNF_ERR_INVALID, std::string(who) + ": nsteps >= 1 required");
    if (alg != CNF_ALG_RK4 && alg != CNF_ALG_TSIT5) return fail(CNF_ERR_INVALID, std::string(who) + ": unknown alg");
    if (!std::isfinite(t0) || !std::isfinite(t1)) return fail(CNF_ERR_INVALID, std::string(who) + ": t0 / t1 must be finite");
    return CNF_OK;
}

}  // namespace

extern "C" {

int cnf_f64_supported(const cnf_handle* h) {
    if (!h) {
        fail(CNF_ERR_INVALID, "cnf_f64_supported: null handle");
        return 0;
    }
    F64Net net;
    const std::string why = f64_refusal(h, &net, 6);   // under every solver
    if (why.empty()) return 1;
    fail(CNF_ERR_UNSUPPORTED, "cnf_f64_supported: " + why);
    return 0;
}

int cnf_set_params_f64(cnf_handle* h, const double* p, size_t n, const size_t* w_off, const size_t* b_off, int p_is_device,
                       void* stream) {
    if (!h || !p || !w_off || !b_off) return fail(CNF_ERR_INVALID, "cnf_set_params_f64: null argument");
    F64Net net;
    const std::string why = f64_refusal(h, &net, 1);   // the least any entry needs (a flow may fit RK4 and not Tsit5: asked per call)
    if (!why.empty()) return fail(CNF_ERR_UNSUPPORTED, "cnf_set_params_f64: " + why);
    const cnf_config& c = h->cfg;
    for (int l = 0; l < c.n_layers; ++l) {
        const size_t wn = (size_t)c.widths[l] * (size_t)c.widths[l + 1];
        if (w_off[l] + wn > n || b_off[l] + (size_t)c.widths[l + 1] > n)
            return fail(CNF_ERR_INVALID, "cnf_set_params_f64: layer offsets exceed the parameter vector");
    }
    DeviceGuard g(c.device_id);
    if (!g.ok) return fail(CNF_ERR_HIP, "cnf_set_params_f64: hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    h->f64.have = false;
    HIP_TRY(h->f64.image.reserve(net.image));
    const double* src = p;
    if (!p_is_device) {
        HIP_TRY(h->f64.lux.reserve(n));
        HIP_TRY(hipMemcpyAsync(h->f64.lux, p, n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));   // the caller may reuse its host buffer on return
        src = h->f64.lux;
    }
    HIP_TRY(f64_pack(net, src, w_off, b_off, h->f64.image, st));
    h->f64.have = true;
    return CNF_OK;
}

int cnf_aug_f_f64(cnf_handle* h, double* du, const double* u, double t, const double* eps, const double* ys, int64_t B,
                  void* stream) {
    F64Net net;
    int rc = check_call(h, &net, 1, eps, ys, B, "cnf_aug_f_f64");
    if (rc) return rc;
    if (B == 0) return CNF_OK;
    if (!du || !u) return fail(CNF_ERR_INVALID, "cnf_aug_f_f64: null u/du");
    if (du == u) return fail(CNF_ERR_INVALID, "cnf_aug_f_f64: du may not alias u");
    DeviceGuard g(h->cfg.device_id);
    F64Args a{};
    a.u0 = u; a.eps = eps; a.ys = ys; a.B = B; a.nsteps = 0; a.t0 = t; a.dt = 0.0;
    a.u_out = du; a.nvars = h->cfg.nvars;
    HIP_TRY(f64_solve(net, h->f64.image, a, (hipStream_t)stream));
    return CNF_OK;
}

int cnf_integrate_fixed_f64(cnf_handle* h, int alg, int nsteps, double t0, double t1, const double* u0, const double* eps,
                            const double* ys, int64_t B, double* u1, void* stream) {
    F64Net net;
    int rc = check_solver(alg, nsteps, t0, t1, "cnf_integrate_fixed_f64");
    if (rc) return rc;
    rc = check_call(h, &net, make_tableau_f64(alg).ns, eps, ys, B, "cnf_integrate_fixed_f64");   // laid out for the solver's own stage count
    if (rc) return rc;
    if (B == 0) return CNF_OK;
    if (!u0 || !u1) return fail(CNF_ERR_INVALID, "cnf_integrate_fixed_f64: null u0/u1");
    DeviceGuard g(h->cfg.device_id);
    F64Args a{};
    a.u0 = u0; a.eps = eps; a.ys = ys; a.B = B; a.nsteps = nsteps; a.t0 = t0; a.dt = (t1 - t0) / (double)nsteps;
    a.u_out = u1; a.nvars = h->cfg.nvars;
    a.T = make_tableau_f64(alg);
    HIP_TRY(f64_solve(net, h->f64.image, a, (hipStream_t)stream));
    return CNF_OK;
}

int cnf_inference_fixed_f64(cnf_handle* h, int alg, int nsteps, double t0, double t1, const double* x, const double* eps,
                            const double* ys, int64_t B, double* logp, double* regs, double* u_final, void* stream) {
    F64Net net;
    int rc = check_solver(alg, nsteps, t0, t1, "cnf_inference_fixed_f64");
    if (rc) return rc;
    rc = check_call(h, &net, make_tableau_f64(alg).ns, eps, ys, B, "cnf_inference_fixed_f64");   // laid out for the solver's own stage count
    if (rc) return rc;
    if (B == 0) return CNF_OK;
    if (!x || !logp) return fail(CNF_ERR_INVALID, "cnf_inference_fixed_f64: null x/logp");
    DeviceGuard g(h->cfg.device_id);
    F64Args a{};
    a.x = x; a.eps = eps; a.ys = ys; a.B = B; a.nsteps = nsteps; a.t0 = t0; a.dt = (t1 - t0) / (double)nsteps;
    a.u_out = u_final; a.logp = logp; a.regs = regs; a.nvars = h->cfg.nvars; a.reg_aug = api_reg_aug(h);
    a.T = make_tableau_f64(alg);
    HIP_TRY(f64_solve(net, h->f64.image, a, (hipStream_t)stream));
    return CNF_OK;
}

}  // extern "C"
