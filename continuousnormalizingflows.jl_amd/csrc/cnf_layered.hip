// cnf_layered.hip — layer-wise evaluation on library GEMMs for what the fused kernels do not cover.
//
// (1) layered_aug_f: the augmented dynamics (SURVEY.md §8 boundary A; src/core/icnf.jl:184-322) for ANY
//     Dense chain — more than four hidden layers, widths above 256, mixed activations, D > 16, several
//     JVP probes — in all three trace modes.  It has the signature of simt_aug_f and plugs into the same
//     RK driver (cnf_api.hip), replacing the thread-per-sample kernels when the batch is large.
// (2) layered_grad: the parameter gradient for every Hutchinson-VJP configuration the fused
//     reverse-sweep kernels (cnf_grad2.hip, cnf_grad2_probes.hip) do not cover: wide layers (BASELINE cfg4,
//     3x256), more than three hidden layers, unequal widths, mixed activations, D > 14.
//
// Same mathematics as cnf_grad.hip (discretise-then-optimise reverse sweep through the fixed-step RK
// solve; reference: Zygote through SciMLBase.solve, src/core/icnf.jl:90-99, objective icnf.jl:184-251,
// 628-637), organised LAYER-WISE over the whole column shard instead of tile-wise: every product is a
// plain product [features x B] on the library's own MFMA kernels (cnf_lgemm.hip), the elementwise pieces ride in their epilogues
// or are the small HIP kernels below.
// With wide layers the arithmetic intensity of these GEMMs is high (256 x 256 x B), so the layer-wise
// form is compute-bound on the matrix cores; the activations of one stage (a_l, act'_l, the pullback
// v_l, ...) live in HBM (cfg4: ~0.6 GB).
//
// Layout: all matrices are column-major [rows x B] = one contiguous column per sample, the layout of
// the ABI's x / eps / ys.  a_l carries an extra row of ones (ld = H_l + 1) and the parameters are kept
// in an augmented copy PA_l = [W_l | b_l] (H_l x (H_{l-1} + 1)), so the bias add is part of the forward
// GEMM and the bias cotangent is the last column of  Wbar_l += sbar_l [a_{l-1}; 1]^T.
//
// Weight cotangents have K = B (tens of thousands) and a small output: they are computed as strided-
// batched GEMMs over column chunks, each chunk accumulating (beta = 1) into its own slab for the whole
// solve; one kernel sums the slabs in a fixed order at the end (no atomics: bit-reproducible).
//
// Activations: every id of cnf.h.  The reverse sweep needs act''_l: tanh, softplus, sigmoid and ELU rebuild it from a_l and
// act'_l (act_dd_rt, cnf_common.h); swish and GELU cannot, so the forward chain of the gradient also writes the pre-activations
// z_l of those layers (ACT epilogue) and act'' is recomputed from z_l.  Extra bytes: 4 H_l B per swish / GELU layer - in the
// recomputing mode once (one stage's worth), in the keep-activations mode per kept stage (4 H_l B x stages x steps, counted
// in the CNF_LAYERED_ACT_GIB budget).  Chains of identity / tanh / softplus keep exactly the workspace they had.
//
// The products run on the hand-written MFMA kernels of cnf_lgemm.hip (weights pre-packed into operand images once per parameter
// set; activation / act' / the pullback's elementwise product fused into their epilogues); the library has no dependency on a
// vendor BLAS.
#include <algorithm>
#include <cstdlib>

#include <string>
#include <vector>

#include "cnf_devbuf.h"
#include "cnf_internal.h"
#include "cnf_coop_grad.h"
#include "cnf_tiles.h"

namespace cnf {

// cnf_lgemm.hip
enum { LG_EPI_PLAIN = 0, LG_EPI_ACT = 1, LG_EPI_MUL = 2, LG_EPI_MUL2 = 3, LG_EPI_BOTTOM = 4, LG_EPI_SBAR = 5 };
hipError_t lg_pack_image(const float* src, long long sm, long long sk, int M, int K, float* img, hipStream_t st);
size_t lg_image_floats(int M, int K);
bool lg_gemm_supported(int M, int K);
hipError_t lg_gemm(const float* img, int M, int K, const float* in, int ldb, float* out, int ldc, long long N, int epi,
                   const float* e, int lde, float* dout, int ldd, int act, hipStream_t st, const float* e2 = nullptr,
                   const float* a3 = nullptr, int ld3 = 0, int first = 0, float* pre = nullptr);
bool lg_wgrad_supported(int M, int Nc);
int lg_wgrad_chunks(int M, long long B, int num_cus, long long* chunk_out, int per_cu_dflt = 2, int Nc = 0);
hipError_t lg_wgrad(float* slabs, long long slab_stride, long long chunk, int nchunks, int M, int Nc, const float* x, int ldx,
                    const float* y, int ldy, long long B, hipStream_t st);

namespace {

struct LDesc {              // the Dense chain, by value in kernel arguments
    int n_layers;
    int win[CNF_MAX_LAYERS], wout[CNF_MAX_LAYERS], act[CNF_MAX_LAYERS];
    long long pa_off[CNF_MAX_LAYERS];   // [W_l | b_l] inside the augmented parameter buffer
    long long w_off[CNF_MAX_LAYERS], b_off[CNF_MAX_LAYERS];   // Lux offsets
    long long npa;
};

constexpr int TPB = 256;
inline dim3 grid_for(long long n) { return dim3((unsigned)((n + TPB - 1) / TPB)); }

// PA_l = [W_l | b_l] gathered from the Lux vector
__global__ void aug_params_kernel(const float* __restrict__ P, float* __restrict__ PA, LDesc L) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.npa) return;
    int l = 0;
    while (l + 1 < L.n_layers && e >= L.pa_off[l + 1]) ++l;
    const long long r = e - L.pa_off[l];
    const int o = (int)(r % L.wout[l]), i = (int)(r / L.wout[l]);
    PA[e] = i < L.win[l] ? P[L.w_off[l] + o + (long long)L.wout[l] * i] : P[L.b_off[l] + o];
}

// grad (Lux layout) = sum of the chunk slabs, fixed order
__global__ void reduce_slabs_kernel(const float* __restrict__ slabs, int nslab, long long stride, LDesc L,
                                    float* __restrict__ grad) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.npa) return;
    // eight independent partial sums (slabs s = k mod 8) keep eight loads in flight; combined in a fixed order (one dependent chain over
    // several hundred slabs took 0.29 ms for the 37 k parameters of the default architecture at nvariables = 20)
    float p8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 8 <= nslab; s += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) p8[k] += slabs[(long long)(s + k) * stride + e];
    }
    for (int k = 0; s < nslab; ++s, ++k) p8[k] += slabs[(long long)s * stride + e];
    const float acc = ((p8[0] + p8[1]) + (p8[2] + p8[3])) + ((p8[4] + p8[5]) + (p8[6] + p8[7]));
    int l = 0;
    while (l + 1 < L.n_layers && e >= L.pa_off[l + 1]) ++l;
    const long long r = e - L.pa_off[l];
    const int o = (int)(r % L.wout[l]), i = (int)(r / L.wout[l]);
    grad[i < L.win[l] ? L.w_off[l] + o + (long long)L.wout[l] * i : L.b_off[l] + o] = acc;
}

// z0 = [x; 0]  (src/core/base_icnf.jl:165-167)
__global__ void init_state_kernel(const float* __restrict__ x, float* __restrict__ z, int nvars, int D, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)D * B) return;
    const long long j = i / D;
    const int f = (int)(i % D);
    z[i] = f < nvars ? x[j * nvars + f] : 0.f;
}

struct Comb { const float* k[6]; float coef[6]; int nk; };
// out = base + sum_j coef_j k_j   (out may alias base)
__global__ void combine_kernel(float* __restrict__ out, const float* __restrict__ base, Comb c, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    for (int j = 0; j < c.nk; ++j) acc = fmaf(c.coef[j], c.k[j][i], acc);
    out[i] = base[i] + acc;
}

// a_0 = [z; t; y; 1]  (CondLayer row order, src/layers/cond_layer.jl:12-23), ld = n_in + 1
__global__ void build_input_kernel(const float* __restrict__ zs, float t, const float* __restrict__ ys,
                                   float* __restrict__ a0, int D, int C, int autonomous, long long B) {
    const int nin = D + (autonomous ? 0 : 1) + C, ld = nin + 1;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)ld * B) return;
    const long long j = i / ld;
    const int f = (int)(i % ld);
    float v;
    if (f < D) v = zs[j * D + f];
    else if (f == nin) v = 1.f;
    else if (!autonomous && f == D) v = t;
    else v = ys[j * C + (f - D - (autonomous ? 0 : 1))];
    a0[i] = v;
}

// dst[rows x B, ld rows] = src[rows x B, ld lds] (first `rows` rows, row offset roff)
__global__ void copy_rows_kernel(float* __restrict__ dst, const float* __restrict__ src, int rows, int lds, int roff, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)rows * B) return;
    const long long j = i / rows;
    const int f = (int)(i % rows);
    dst[i] = src[j * lds + roff + f];
}

// seed of the exact trace: the unit vector e_k in every column (tr J = sum_k e_k^T J e_k)
__global__ void onehot_kernel(float* __restrict__ dst, int k, int D, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long long)D * B) dst[i] = (int)(i % D) == k ? 1.f : 0.f;
}

__global__ void mul_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[i] * y[i];
}

// kbar = dt (b lam + sum_j a_j Zb_j)  (+ cE zdot / |zdot|: Edot = |zdot|, src/core/icnf.jl:184-199)
// cw (null: the shipped loss, whose row cotangents are the uniform scalars): per-column cotangents of the dlogp / E / n rows, column j
// at cw[j ldw + 0..2] (the pullback of the solve) - cE, and cl / cn in the gbar kernels, are then multiplied by the column's entry
__global__ void kbar_kernel(float* __restrict__ kbar, const float* __restrict__ lam, Comb zb, float dtb, float dt,
                            const float* __restrict__ aN, float cE, int D, long long B, const float* __restrict__ cw = nullptr, int ldw = 0) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float inv = 0.f;
    if (cE != 0.f) {
        float e2 = 0.f;
        for (int f = 0; f < D; ++f) { const float v = aN[j * (D + 1) + f]; e2 = fmaf(v, v, e2); }
        inv = e2 > 0.f ? cE * rsqrtf(e2) : 0.f;
        if (cw) inv *= cw[j * ldw + 1];
    }
    for (int f = 0; f < D; ++f) {
        float acc = 0.f;
        for (int q = 0; q < zb.nk; ++q) acc = fmaf(zb.coef[q], zb.k[q][j * D + f], acc);
        float v = fmaf(dtb, lam[j * D + f], dt * acc);
        if (cE != 0.f) v = fmaf(inv, aN[j * (D + 1) + f], v);
        kbar[j * D + f] = v;
    }
}

// gbar = -c_l eps_k + c_n g / |g|   (cotangent of g = eps^T J; ldot = -<eps, g>/K, ndot = |g|/K)
__global__ void gbar_kernel(float* __restrict__ gbar, const float* __restrict__ g, const float* __restrict__ epsk,
                            float cl, float cn, int D, long long B, const float* __restrict__ cw = nullptr, int ldw = 0) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float inv = 0.f;
    if (cn != 0.f) {
        float n2 = 0.f;
        for (int f = 0; f < D; ++f) { const float v = g[j * D + f]; n2 = fmaf(v, v, n2); }
        inv = n2 > 0.f ? cn * rsqrtf(n2) : 0.f;
    }
    if (cw) { cl *= cw[j * ldw]; inv *= cw[j * ldw + 2]; }
    for (int f = 0; f < D; ++f) gbar[j * D + f] = fmaf(inv, g[j * D + f], -cl * epsk[j * D + f]);
}

// The loss of the same discrete solve, accumulated stage by stage in the reverse sweep (the stage's zdot and eps^T J are at
// hand there): E += w |zdot|;  dlogp += wl <eps_k, g_k>;  n += wn |g_k|
__global__ void loss_acc_z_kernel(float* __restrict__ eacc, const float* __restrict__ aN, int ldn, float w, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float n2 = 0.f;
    for (int f = 0; f < D; ++f) { const float v = aN[j * ldn + f]; n2 = fmaf(v, v, n2); }
    eacc[j] = fmaf(w, sqrtf(n2), eacc[j]);
}
__global__ void loss_acc_g_kernel(float* __restrict__ lacc, float* __restrict__ nacc, const float* __restrict__ g,
                                  const float* __restrict__ epsk, float wl, float wn, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float dot = 0.f, n2 = 0.f;
    for (int f = 0; f < D; ++f) { const float v = g[j * D + f]; dot = fmaf(epsk[j * D + f], v, dot); n2 = fmaf(v, v, n2); }
    lacc[j] = fmaf(wl, dot, lacc[j]);
    if (wn != 0.f) nacc[j] = fmaf(wn, sqrtf(n2), nacc[j]);
}
// u = [z; dlogp; E; n] per column
__global__ void pack_final_kernel(float* __restrict__ u, const float* __restrict__ z, const float* __restrict__ lacc,
                                  const float* __restrict__ eacc, const float* __restrict__ nacc, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    const int S = D + 3;
    for (int f = 0; f < D; ++f) u[j * S + f] = z[j * D + f];
    u[j * S + D] = lacc[j]; u[j * S + D + 1] = eacc[j]; u[j * S + D + 2] = nacc[j];
}

// ---- the same per-column kernels with one lane per (column, feature): G = the power of two >= D (<= 64) lanes share a
// column, loads and stores are coalesced (the thread-per-column forms above walk a column with stride-D accesses and
// occupy half the chip at B = 32 K: 12-20 us each, five of them per stage), norms and dots are butterfly sums over the group
__device__ __forceinline__ float group_sum_w(float v, int G) {
    for (int o = G >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
__global__ void kbar_grp_kernel(float* __restrict__ kbar, const float* __restrict__ lam, Comb zb, float dtb, float dt,
                                const float* __restrict__ aN, float cE, int D, int G, long long B, const float* __restrict__ cw = nullptr, int ldw = 0) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j = i / G;
    const int f = (int)(i % G);
    const bool ok = j < B && f < D;
    float z = ok ? aN[j * (D + 1) + f] : 0.f;
    float inv = 0.f;
    if (cE != 0.f) {
        const float e2 = group_sum_w(z * z, G);
        inv = e2 > 0.f ? cE * rsqrtf(e2) : 0.f;
        if (cw && ok) inv *= cw[j * ldw + 1];
    }
    if (!ok) return;
    float acc = 0.f;
    for (int q = 0; q < zb.nk; ++q) acc = fmaf(zb.coef[q], zb.k[q][j * D + f], acc);
    float v = fmaf(dtb, lam[j * D + f], dt * acc);
    if (cE != 0.f) v = fmaf(inv, z, v);
    kbar[j * D + f] = v;
}
__global__ void gbar_grp_kernel(float* __restrict__ gbar, const float* __restrict__ g, const float* __restrict__ epsk,
                                float cl, float cn, float* __restrict__ lacc, float* __restrict__ nacc, float wl, float wn,
                                int D, int G, long long B, const float* __restrict__ cw = nullptr, int ldw = 0) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j = i / G;
    const int f = (int)(i % G);
    const bool ok = j < B && f < D;
    const float gv = ok ? g[j * D + f] : 0.f, ev = ok ? epsk[j * D + f] : 0.f;
    float inv = 0.f, n2 = 0.f;
    if (cn != 0.f || (lacc && wn != 0.f)) n2 = group_sum_w(gv * gv, G);
    if (cn != 0.f) inv = n2 > 0.f ? cn * rsqrtf(n2) : 0.f;
    if (lacc) {     // the loss terms of this stage and probe ride along: dlogp += wl <eps, g>, n += wn |g|
        const float dot = group_sum_w(ev * gv, G);
        if (ok && f == 0) {
            lacc[j] = fmaf(wl, dot, lacc[j]);
            if (wn != 0.f) nacc[j] = fmaf(wn, sqrtf(n2), nacc[j]);
        }
    }
    if (cw && ok) { cl *= cw[j * ldw]; inv *= cw[j * ldw + 2]; }
    if (ok) gbar[j * D + f] = fmaf(inv, gv, -cl * ev);
}
__global__ void loss_acc_z_grp_kernel(float* __restrict__ eacc, const float* __restrict__ aN, int ldn, float w, int D, int G, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j = i / G;
    const int f = (int)(i % G);
    const bool ok = j < B && f < D;
    const float v = ok ? aN[j * ldn + f] : 0.f;
    const float n2 = group_sum_w(v * v, G);
    if (ok && f == 0) eacc[j] = fmaf(w, sqrtf(n2), eacc[j]);
}

// vbar = dbar .* act';  acc2 += dbar .* v
__global__ void bottom_kernel(const float* __restrict__ db, const float* __restrict__ d, const float* __restrict__ v,
                              float* __restrict__ vbar, float* __restrict__ acc2, int first, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = db[i];
    vbar[i] = x * d[i];
    acc2[i] = first ? x * v[i] : fmaf(x, v[i], acc2[i]);   // the first probe initialises the sum
}

// sbar = abar .* act' + acc2 .* act''   (act'' = act_dd_rt(act, x, act'): x the activations a (ld H + 1; tanh: act'' = -2 a act'),
// or the pre-activations (ld H) of swish / GELU)
__global__ void sbar_kernel(float* __restrict__ sbar, const float* __restrict__ abar, const float* __restrict__ d,
                            const float* __restrict__ acc2, const float* __restrict__ x, int ldx, int act, int H, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)H * B) return;
    const long long j = i / H;
    const int f = (int)(i % H);
    const float dd = d[i];
    const float e = act_dd_rt(act, act_dd_reads_x(act) ? x[j * ldx + f] : 0.f, dd);
    sbar[i] = fmaf(acc2[i], e, abar[i] * dd);
}

// lam_N = dL/dz_N = z_N (+ l3 z_aug / |z_aug|, src/core/base_icnf.jl:106-122)
__global__ void lam_init_kernel(float* __restrict__ lam, const float* __restrict__ zN, float lam3, int nvars, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float inv = 0.f;
    if (lam3 != 0.f) {
        float s = 0.f;
        for (int f = nvars; f < D; ++f) { const float v = zN[j * D + f]; s = fmaf(v, v, s); }
        inv = s > 0.f ? lam3 * rsqrtf(s) : 0.f;
    }
    for (int f = 0; f < D; ++f) {
        const float v = zN[j * D + f];
        lam[j * D + f] = f >= nvars ? fmaf(inv, v, v) : v;
    }
}

// the pullback of the solve: the dlogp / E / n accumulators start from rows D .. D+2 of u0 (S x B), not from zero
__global__ void cot_rows_init_kernel(float* __restrict__ lacc, float* __restrict__ eacc, float* __restrict__ nacc,
                                     const float* __restrict__ u0, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    const int S = D + 3;
    lacc[j] = u0[j * S + D]; eacc[j] = u0[j * S + D + 1]; nacc[j] = u0[j * S + D + 2];
}
// u0_bar = [costate at t0; rows D .. D+2 of u1_bar] (those rows feed nothing: passed through)
__global__ void cot_out_kernel(float* __restrict__ u0_bar, const float* __restrict__ lam, const float* __restrict__ u1_bar, int D, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = D + 3;
    if (i >= (long long)S * B) return;
    const long long j = i / S;
    const int f = (int)(i % S);
    u0_bar[i] = f < D ? lam[j * D + f] : u1_bar[i];
}

// ---- forward evaluation (layered_aug_f) ----

// a_0 = [z; t; y; 1] with z = rows 0..D-1 of  u + dt sum_j coef_j k_j  (state layout S x B)
__global__ void build_input_stage_kernel(StageIn in, int S, float t, const float* __restrict__ ys, float* __restrict__ a0,
                                         int D, int C, int autonomous, long long B) {
    const int nin = D + (autonomous ? 0 : 1) + C, ld = nin + 1;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)ld * B) return;
    const long long j = i / ld;
    const int f = (int)(i % ld);
    float v;
    if (f < D) {
        float acc = 0.f;
        for (int q = 0; q < in.nprev; ++q) acc = fmaf(in.coef[q], in.k[q][j * S + f], acc);
        v = fmaf(in.dt, acc, in.u[j * S + f]);
    } else if (f == nin) v = 1.f;
    else if (!autonomous && f == D) v = t;
    else v = ys[j * C + (f - D - (autonomous ? 0 : 1))];
    a0[i] = v;
}

// out[rows x B] = x[rows roff.. of ld ldx] .* y[rows x B]
__global__ void mul_rows_kernel(float* __restrict__ out, const float* __restrict__ x, int ldx, int roff,
                                const float* __restrict__ y, int rows, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)rows * B) return;
    const long long j = i / rows;
    const int f = (int)(i % rows);
    out[i] = x[j * ldx + roff + f] * y[i];
}

// Hutchinson accumulation for one probe: ldot -= scale <g, eps_k>;  ndot += scale |g|   (icnf.jl:229-245)
__global__ void trace_kernel(const float* __restrict__ g, const float* __restrict__ eps, int lde, int roff,
                             float* __restrict__ ld, float* __restrict__ nd, float scale, int reg_j, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float dot = 0.f, n2 = 0.f;
    for (int f = 0; f < D; ++f) {
        const float gv = g[j * D + f];
        dot = fmaf(gv, eps[j * lde + roff + f], dot);
        n2 = fmaf(gv, gv, n2);
    }
    ld[j] -= scale * dot;
    if (reg_j) nd[j] += scale * sqrtf(n2);
}

// exact trace, unit tangent e_i: tau_1 = W_1[:, i] .* act'_1
__global__ void exact_seed_kernel(float* __restrict__ tau, const float* __restrict__ w1col, const float* __restrict__ d1,
                                  int H, long long B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)H * B) return;
    tau[i] = w1col[i % H] * d1[i];
}

// row[j] = <w (stride ws), tau[:, j]>: row i of W_N applied to one tangent per column (a 1 x B product: one wave per column,
// lanes over the H entries, so the loads of a column are coalesced; an MFMA tile would waste 15 of its 16 rows)
__global__ void rowdot_kernel(const float* __restrict__ w, long long ws, const float* __restrict__ tau, int H, float* __restrict__ row,
                              long long B) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long j = wave; j < B; j += nwaves) {
        float acc = 0.f;
        for (int k = lane; k < H; k += 64) acc = fmaf(w[(long long)k * ws], tau[j * H + k], acc);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) row[j] = acc;
    }
}

// ldot -= act'_N[i] * (W_N[i, :] tau)   (J_ii)
__global__ void exact_diag_kernel(const float* __restrict__ row, const float* __restrict__ dN, int D, int i,
                                  float* __restrict__ ld, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < B) ld[j] -= row[j] * dN[j * D + i];
}

// Two hidden layers: Q[a][b] = W_2[a][b] * sum_i W_1[b][i] W_3[i][a]  (tr J = act'_2^T Q act'_1; see mfma_pack / pack_q_kernel)
__global__ void layered_q_kernel(const float* __restrict__ PA, float* __restrict__ Q, LDesc L, int D) {
    const int H1 = L.wout[0], H2 = L.wout[1];
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)H1 * H2) return;
    const int a = (int)(e % H2), b = (int)(e / H2);      // Q column-major (H2 x H1)
    const float* W1 = PA + L.pa_off[0];
    const float* W2 = PA + L.pa_off[1];
    const float* W3 = PA + L.pa_off[2];
    double acc = 0.0;
    for (int i = 0; i < D; ++i) acc += (double)W1[b + (long long)H1 * i] * (double)W3[i + (long long)D * a];
    Q[e] = (float)((double)W2[a + (long long)H2 * b] * acc);
}

// ldot = -<q_j, act'_2[:, j]> per column
__global__ void neg_coldot_kernel(const float* __restrict__ x, const float* __restrict__ y, int rows, float* __restrict__ ld, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    float acc = 0.f;
    for (int f = 0; f < rows; ++f) acc = fmaf(x[j * rows + f], y[j * rows + f], acc);
    ld[j] = -acc;
}

// du = [zdot; ldot; |zdot| (reg_z); ndot]
__global__ void finish_kernel(float* __restrict__ du, const float* __restrict__ aN, const float* __restrict__ ld,
                              const float* __restrict__ nd, int reg_z, int D, long long B) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    const int S = D + 3;
    float e2 = 0.f;
    for (int f = 0; f < D; ++f) {
        const float v = aN[j * (D + 1) + f];
        du[j * S + f] = v;
        e2 = fmaf(v, v, e2);
    }
    du[j * S + D] = ld[j];
    du[j * S + D + 1] = reg_z ? sqrtf(e2) : 0.f;
    du[j * S + D + 2] = nd[j];
}

}  // namespace

// an operand image of A(m, k) = PA[rel + m * sm + k * sk] (M x K), repacked whenever the parameters change
struct LgImage {
    long long rel, sm, sk;
    int M, K;
    DevBuf<float> img;
    unsigned epoch = 0;
};

struct LayeredGrad {
    std::vector<LgImage> images;
    unsigned epoch = 1;           // bumped whenever PA is rebuilt: stale images are repacked at their next use
    int num_cus = 0;
    DevBuf<float> ws;             // gradient workspace
    DevBuf<float> ws_fwd;         // forward-evaluation workspace (the gradient calls the forward for the loss)
    DevBuf<float> ws_store;       // the stage store of the cooperative gradient's second form (cnf_tiles.h): h_l, delta_l of every stage
};

void layered_grad_destroy(LayeredGrad* g) { delete g; }

bool layered_grad_supported(const cnf_config& c) {
    return c.mode == CNF_MODE_EXACT || ((c.mode == CNF_MODE_HUTCH_VJP || c.mode == CNF_MODE_HUTCH_JVP) && c.nprobes >= 1);
}

#define LG_HIP(expr)                                                                    \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) { *err = std::string(#expr) + ": " + hipGetErrorString(_e); return _e; } \
    } while (0)
#define LG_BLAS(expr) LG_HIP(expr)

// G.num_cus of the current device, asked on first use
static hipError_t lg_num_cus(LayeredGrad& G, std::string* err) {
    if (G.num_cus != 0) return hipSuccess;
    int dev = 0;
    hipDeviceProp_t prop;
    LG_HIP(hipGetDevice(&dev));
    LG_HIP(hipGetDeviceProperties(&prop, dev));
    G.num_cus = prop.multiProcessorCount;
    return hipSuccess;
}

// the Dense chain of `c` with its Lux offsets; [W_l | b_l] blocks back to back in the augmented parameter buffer
static LDesc make_ldesc(const cnf_config& c, const size_t* w_off, const size_t* b_off) {
    LDesc L{};
    L.n_layers = c.n_layers;
    long long npa = 0;
    for (int l = 0; l < c.n_layers; ++l) {
        L.win[l] = c.widths[l]; L.wout[l] = c.widths[l + 1]; L.act[l] = c.acts[l];
        L.pa_off[l] = npa; L.w_off[l] = (long long)w_off[l]; L.b_off[l] = (long long)b_off[l];
        npa += (long long)L.wout[l] * (L.win[l] + 1);
    }
    L.npa = npa;
    return L;
}
static int max_width(const LDesc& L, int D) {
    int maxw = D;
    for (int l = 0; l < L.n_layers; ++l)
        if (L.wout[l] > maxw) maxw = L.wout[l];
    return maxw;
}

// carves a workspace into arrays that start on 64-float boundaries: take(n) is the offset of the next one, `off` the floats taken so far
struct Carver {
    long long off = 0;
    long long operator()(long long n) {
        const long long o = off;
        off += (n + 63) / 64 * 64;
        return o;
    }
};

// every product of the chain (forward, transposed, weight cotangent) fits one launch of the kernels in cnf_lgemm.hip
bool layered_available() { return true; }
bool layered_supports(const cnf_config& c) {
    for (int l = 0; l < c.n_layers; ++l) {
        const int win = c.widths[l], wout = c.widths[l + 1];
        if (!lg_gemm_supported(wout, win + 1) || !lg_gemm_supported(win, wout) || !lg_wgrad_supported(wout, win + 1)) return false;
    }
    return true;
}

// the image of A(m, k) = PA[rel + m sm + k sk], packed on first use and again after every parameter rebuild
static hipError_t lg_image(LayeredGrad& G, const float* PA, long long rel, long long sm, long long sk, int M, int K,
                           const float** out, hipStream_t st) {
    for (LgImage& im : G.images) {
        if (im.rel == rel && im.sm == sm && im.sk == sk && im.M == M && im.K == K) {
            if (im.epoch != G.epoch) {
                hipError_t e = lg_pack_image(PA + rel, sm, sk, M, K, im.img, st);
                if (e != hipSuccess) return e;
                im.epoch = G.epoch;
            }
            *out = im.img;
            return hipSuccess;
        }
    }
    LgImage im;
    im.rel = rel; im.sm = sm; im.sk = sk; im.M = M; im.K = K;
    hipError_t e = im.img.reserve(lg_image_floats(M, K));
    if (e != hipSuccess) return e;
    e = lg_pack_image(PA + rel, sm, sk, M, K, im.img, st);
    if (e != hipSuccess) return e;
    im.epoch = G.epoch;
    *out = im.img;
    G.images.push_back(std::move(im));
    return hipSuccess;
}

// C (ldc) = op(A) Bm: A = PA + rel (column-major m x k with lda, or its transpose) - the call shape of the BLAS routine this
// replaces; epi / e / dout select the fused epilogue (LG_EPI_*)
enum { OPN = 0, OPT = 1 };
static hipError_t lg_product(LayeredGrad& G, const float* PA, int ta, int m, long long n, int k, const float* A, int lda,
                             const float* Bm, int ldb, float* Cm, int ldc, int epi, const float* e, int lde, float* dout, int ldd,
                             int act, hipStream_t st, const float* e2 = nullptr, const float* a3 = nullptr, int ld3 = 0,
                             int first = 0, float* pre = nullptr) {
    if (!lg_gemm_supported(m, k)) return hipErrorNotSupported;
    const float* img = nullptr;
    const long long rel = A - PA;
    hipError_t er = ta == OPN ? lg_image(G, PA, rel, 1, lda, m, k, &img, st) : lg_image(G, PA, rel, lda, 1, m, k, &img, st);
    if (er != hipSuccess) return er;
    return lg_gemm(img, m, k, Bm, ldb, Cm, ldc, n, epi, e, lde, dout, ldd, act, st, e2, a3, ld3, first, pre);
}

// du = augmented_f(u + dt sum coef k, p, t): forward chain, then the trace estimator of the handle's mode
hipError_t layered_aug_f(LayeredGrad** ctx, const cnf_config& c, const float* P_dev, const size_t* w_off,
                         const size_t* b_off, bool rebuild_params, const StageIn& in, float t, const float* eps,
                         const float* ys, long long B, float* du, hipStream_t st, std::string* err) {
    if (!layered_supports(c)) {
        *err = "layered evaluation: a layer is wider than the product kernels cover (512 outputs, 639 inputs)";
        return hipErrorNotSupported;
    }
    for (int l = 0; l < c.n_layers; ++l)
        if (!act_id_valid(c.acts[l])) {
            *err = "layered evaluation: unknown activation id";
            return hipErrorInvalidValue;
        }
    if (!*ctx) *ctx = new LayeredGrad();
    LayeredGrad& G = **ctx;
    const int N = c.n_layers, D = c.nvars + c.naug, C = c.ncond, S = D + 3;
    const int K = c.mode == CNF_MODE_EXACT ? 1 : c.nprobes;
    const LDesc L = make_ldesc(c, w_off, b_off);
    const long long npa = L.npa;
    const int maxw = max_width(L, D);
    Carver take;
    const long long o_PA = take(npa);
    const bool use_q = c.mode == CNF_MODE_EXACT && N == 3 && c.acts[2] == CNF_ACT_IDENTITY;   // two hidden layers
    const long long o_Q = take(use_q ? (long long)L.wout[0] * L.wout[1] : 0);
    long long o_a[CNF_MAX_LAYERS + 1], o_d[CNF_MAX_LAYERS];
    o_a[0] = take((long long)(c.widths[0] + 1) * B);
    for (int l = 0; l < N; ++l) { o_a[l + 1] = take((long long)(L.wout[l] + 1) * B); o_d[l] = take((long long)L.wout[l] * B); }
    const long long WB = (long long)maxw * B;
    const long long o_t0 = take(WB), o_t1 = take(WB), o_ld = take(B), o_nd = take(B), o_row = take(B);
    bool grown = false;   // a workspace that moved has lost its parameter image
    LG_HIP(G.ws_fwd.reserve((size_t)take.off, &grown));
    float* W = G.ws_fwd;
    float* PA = W + o_PA;
    float *a[CNF_MAX_LAYERS + 1], *d[CNF_MAX_LAYERS];
    for (int l = 0; l <= N; ++l) a[l] = W + o_a[l];
    for (int l = 0; l < N; ++l) d[l] = W + o_d[l];
    float *tA = W + o_t0, *tB = W + o_t1, *ldacc = W + o_ld, *ndacc = W + o_nd, *row = W + o_row;
    float* Qm = W + o_Q;
    if (rebuild_params || grown) {
        hipLaunchKernelGGL(aug_params_kernel, grid_for(npa), dim3(TPB), 0, st, P_dev, PA, L);
        if (use_q) hipLaunchKernelGGL(layered_q_kernel, grid_for((long long)L.wout[0] * L.wout[1]), dim3(TPB), 0, st, PA, Qm, L, D);
        ++G.epoch;   // operand images of the old parameters are repacked at their next use
    }

    // C = op(A) Bm (plain), and the two fused forms: .* e, and activation (h, act', ones row)
    auto gemm = [&](int ta, int, int m, long long n, int k, const float* A, int lda, const float* Bm, int ldb, float* Cm,
                    int ldc) -> hipError_t {
        return lg_product(G, PA, ta, m, n, k, A, lda, Bm, ldb, Cm, ldc, LG_EPI_PLAIN, nullptr, 0, nullptr, 0, 0, st);
    };
    auto gemm_mul = [&](int ta, int m, long long n, int k, const float* A, int lda, const float* Bm, int ldb, float* Cm, int ldc,
                        const float* e, int lde) -> hipError_t {
        return lg_product(G, PA, ta, m, n, k, A, lda, Bm, ldb, Cm, ldc, LG_EPI_MUL, e, lde, nullptr, 0, 0, st);
    };

    // forward chain
    hipLaunchKernelGGL(build_input_stage_kernel, grid_for((long long)(c.widths[0] + 1) * B), dim3(TPB), 0, st, in, S, t, ys, a[0],
                       D, C, c.autonomous, B);
    for (int l = 0; l < N; ++l)   // a_{l+1} = act(W_l a_l + b_l) with act' and the ones row, one launch
        LG_BLAS(lg_product(G, PA, OPN, L.wout[l], B, L.win[l] + 1, PA + L.pa_off[l], L.wout[l], a[l], L.win[l] + 1, a[l + 1],
                           L.wout[l] + 1, LG_EPI_ACT, nullptr, 0, d[l], L.wout[l], L.act[l], st));
    LG_HIP(zero_async(ldacc, (size_t)B * sizeof(float), st));
    LG_HIP(zero_async(ndacc, (size_t)B * sizeof(float), st));

    if (c.mode == CNF_MODE_HUTCH_VJP) {
        // g = eps^T J: delta_N = eps .* act'_N, delta_{l-1} = (W_l^T delta_l) .* act'_{l-1}, g = W_1[:,0:D]^T delta_1
        for (int k = 0; k < K; ++k) {
            float *dl = tA, *vv = tB;
            hipLaunchKernelGGL(mul_rows_kernel, grid_for((long long)D * B), dim3(TPB), 0, st, dl, eps, K * D, k * D, d[N - 1], D, B);
            for (int l = N - 1; l >= 1; --l) {
                LG_BLAS(gemm_mul(OPT, L.win[l], B, L.wout[l], PA + L.pa_off[l], L.wout[l], dl, L.wout[l], vv, L.win[l], d[l - 1], L.win[l]));
                float* tmp = dl; dl = vv; vv = tmp;
            }
            LG_BLAS(gemm(OPT, OPN, D, B, L.wout[0], PA, L.wout[0], dl, L.wout[0], vv, D));
            hipLaunchKernelGGL(trace_kernel, grid_for(B), dim3(TPB), 0, st, vv, eps, K * D, k * D, ldacc, ndacc, 1.f / (float)K,
                               c.reg_j, D, B);
        }
    } else if (c.mode == CNF_MODE_HUTCH_JVP) {
        // g = J eps: tau_1 = (W_1[:,0:D] eps) .* act'_1, tau_{l+1} = (W_{l+1} tau_l) .* act'_{l+1}
        for (int k = 0; k < K; ++k) {
            float *tau = tA, *nx = tB;
            LG_BLAS(gemm_mul(OPN, L.wout[0], B, D, PA, L.wout[0], eps + (long long)k * D, K * D, tau, L.wout[0], d[0], L.wout[0]));
            for (int l = 1; l < N; ++l) {
                LG_BLAS(gemm_mul(OPN, L.wout[l], B, L.win[l], PA + L.pa_off[l], L.wout[l], tau, L.win[l], nx, L.wout[l], d[l], L.wout[l]));
                float* tmp = tau; tau = nx; nx = tmp;
            }
            hipLaunchKernelGGL(trace_kernel, grid_for(B), dim3(TPB), 0, st, tau, eps, K * D, k * D, ldacc, ndacc, 1.f / (float)K,
                               c.reg_j, D, B);
        }
    } else if (use_q) {
        // two hidden layers: tr J = act'_2^T Q act'_1 - one GEMM and a column dot instead of D tangent passes
        LG_BLAS(gemm(OPN, OPN, L.wout[1], B, L.wout[0], Qm, L.wout[1], d[0], L.wout[0], tA, L.wout[1]));
        hipLaunchKernelGGL(neg_coldot_kernel, grid_for(B), dim3(TPB), 0, st, tA, d[1], L.wout[1], ldacc, B);
    } else {
        // exact trace: unit tangents e_i pushed forward, J_ii read off the i-th output row (icnf.jl:312)
        for (int i = 0; i < D; ++i) {
            float *tau = tA, *nx = tB;
            if (N == 1) {
                // single layer: J_ii = act'_1[i] W_1[i, i]
                hipLaunchKernelGGL(copy_rows_kernel, grid_for(B), dim3(TPB), 0, st, row, PA + i + (long long)L.wout[0] * i, 1, 0, 0, B);
            } else {
                hipLaunchKernelGGL(exact_seed_kernel, grid_for((long long)L.wout[0] * B), dim3(TPB), 0, st, tau,
                                   PA + (long long)L.wout[0] * i, d[0], L.wout[0], B);
                for (int l = 1; l < N - 1; ++l) {
                    LG_BLAS(gemm_mul(OPN, L.wout[l], B, L.win[l], PA + L.pa_off[l], L.wout[l], tau, L.win[l], nx, L.wout[l], d[l], L.wout[l]));
                    float* tmp = tau; tau = nx; nx = tmp;
                }
                // row i of W_N tau: a 1 x B product
                hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)std::min<long long>((B + 3) / 4, 4096)), dim3(TPB), 0, st,
                                   PA + L.pa_off[N - 1] + i, (long long)L.wout[N - 1], tau, L.win[N - 1], row, B);
            }
            hipLaunchKernelGGL(exact_diag_kernel, grid_for(B), dim3(TPB), 0, st, row, d[N - 1], D, i, ldacc, B);
        }
    }
    hipLaunchKernelGGL(finish_kernel, grid_for(B), dim3(TPB), 0, st, du, a[N], ldacc, ndacc, c.reg_z, D, B);
    LG_HIP(hipGetLastError());
    return hipSuccess;
}

hipError_t layered_grad(LayeredGrad** ctx, const cnf_config& c, const float* P_dev, const size_t* w_off,
                        const size_t* b_off, const float* x, const float* eps, const float* ys, int alg,
                        int nsteps, float t0, float t1, const float* tgrid, long long B, const float lam[3], float* grad,
                        float* grad_x, hipStream_t st, std::string* err, float* logp_out, float* regs_out, const LayeredCot* cot) {
    if (!layered_supports(c)) {
        *err = "layered gradient: a layer is wider than the product kernels cover (512 outputs, 639 inputs)";
        return hipErrorNotSupported;
    }
    for (int l = 0; l < c.n_layers; ++l)
        if (!act_id_valid(c.acts[l])) {   // (act_dd_rt has no act'' for it)
            *err = "layered gradient: unknown activation id";
            return hipErrorInvalidValue;
        }
    if (!*ctx) *ctx = new LayeredGrad();
    LayeredGrad& G = **ctx;
    if (hipError_t e = lg_num_cus(G, err)) return e;

    // TestMode (icnf.jl:297-339): ldot = -tr J = -sum_k e_k^T J e_k - the pullback below with the D unit vectors as
    // probes, each with weight 1 (what the reference's AD does through its D one-hot passes)
    const bool exact = c.mode == CNF_MODE_EXACT;
    const int N = c.n_layers, D = c.nvars + c.naug, C = c.ncond, K = exact ? D : c.nprobes;
    const LDesc L = make_ldesc(c, w_off, b_off);
    const long long npa = L.npa;
    const int maxw = max_width(L, D);
    const long long npa_pad = (npa + 63) / 64 * 64;
    // sample chunks of the weight-cotangent products: one slab per chunk, each chunk's strip of C accumulated in registers
    // (cnf_lgemm.hip); CNF_LAYERED_KC overrides the chunk length
    long long kc = 0;
    int nslab = lg_wgrad_chunks(maxw, B, G.num_cus, &kc);
    if (tuning().layered_kc >= 16) { kc = ((long long)tuning().layered_kc + 3) / 4 * 4; nslab = (int)((B + kc - 1) / kc); }

    // ---- workspace ----
    const long long DB = (long long)D * B;
    Carver take;
    const long long o_PA = take(npa_pad), o_slab = take(npa_pad * nslab), o_zck = take(DB * (nsteps + 1));
    // stage derivatives of every step are kept when they fit 4 GiB, otherwise recomputed in the reverse sweep
    const int nst = alg == CNF_ALG_RK4 ? 4 : 6;
    const bool keep_k = (double)DB * nst * nsteps * sizeof(float) <= 4.0 * 1024 * 1024 * 1024 && !tuning().layered_no_kckpt;
    const long long o_kck = keep_k ? take(DB * nst * nsteps) : 0;
    // the activations of every stage (a_l with its ones row, act'_l) are kept too when they fit the budget (default 48 GiB of
    // the 288; CNF_LAYERED_ACT_GIB): the reverse sweep then reads them instead of recomputing the forward chain of the stage
    // (swish / GELU layers keep their pre-activations z_l as well: act'' is not a function of a_l and act'_l there)
    long long act_stage = (long long)(c.widths[0] + 1) * B;
    int npre = 0;
    for (int l = 0; l < N; ++l) {
        act_stage += (long long)(L.wout[l] + 1) * B + (long long)L.wout[l] * B;
        if (act_dd_needs_pre(L.act[l])) { act_stage += (long long)L.wout[l] * B; ++npre; }
    }
    act_stage = (act_stage + 63) / 64 * 64 + 64 * (N + 2) * 2 + 64 * npre;
    const double act_gib = (double)tuning().layered_act_gib;
    bool keep_act = keep_k && (double)act_stage * nst * nsteps * sizeof(float) <= act_gib * 1024.0 * 1024.0 * 1024.0;
    if (keep_act) {   // ... and half of what the device has free (counting the workspace this context already holds)
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) { (void)hipGetLastError(); mfree = 0; }
        const double avail = (double)mfree + (double)G.ws.capacity() * sizeof(float);
        if ((double)act_stage * nst * nsteps * sizeof(float) > 0.5 * avail) keep_act = false;
    }
    const long long o_actck = keep_act ? take(act_stage * nst * nsteps) : 0;
    long long o_kz[6], o_zb[6];
    for (int j = 0; j < 6; ++j) o_kz[j] = take(DB);
    for (int j = 0; j < 6; ++j) o_zb[j] = take(DB);
    const long long o_lacc = take(3 * B), o_ufin = take((long long)(D + 3) * B);
    const long long o_lam = take(DB), o_kbar = take(DB), o_zs = take(DB), o_g = take(DB), o_gbar = take(DB), o_vN = take(DB);
    long long o_a[CNF_MAX_LAYERS + 1], o_d[CNF_MAX_LAYERS], o_v[CNF_MAX_LAYERS], o_acc2[CNF_MAX_LAYERS], o_dl[CNF_MAX_LAYERS];
    o_a[0] = take((long long)(c.widths[0] + 1) * B);
    for (int l = 0; l < N; ++l) {
        const long long HB = (long long)L.wout[l] * B;
        o_a[l + 1] = take((long long)(L.wout[l] + 1) * B);
        o_d[l] = take(HB); o_v[l] = take(HB); o_acc2[l] = take(HB); o_dl[l] = take(HB);
    }
    const long long WB = (long long)maxw * B;
    const long long o_t0 = take(WB), o_t1 = take(WB), o_t2 = take(WB), o_t3 = take(WB), o_t4 = take(WB);
    long long o_z[CNF_MAX_LAYERS];   // pre-activations of the swish / GELU layers (recomputing mode; nothing for other layers)
    for (int l = 0; l < N; ++l) o_z[l] = act_dd_needs_pre(L.act[l]) && !keep_act ? take((long long)L.wout[l] * B) : -1;
    // the pullback with ys_bar: the sum over all stages of sbar_1 (H_1 x B), taken last so that every other region keeps its place
    float* const ys_bar = (cot && C > 0) ? cot->ys_bar : nullptr;
    const long long H1B = (long long)L.wout[0] * B;
    const long long o_ysum = ys_bar ? take(H1B) : 0;
    LG_HIP(G.ws.reserve((size_t)take.off));
    float* W = G.ws;
    float* PA = W + o_PA;
    float* slabs = W + o_slab;
    float *kz[6], *Zb[6], *a[CNF_MAX_LAYERS + 1], *d[CNF_MAX_LAYERS], *v[CNF_MAX_LAYERS], *acc2[CNF_MAX_LAYERS], *dl[CNF_MAX_LAYERS];
    for (int j = 0; j < 6; ++j) { kz[j] = W + o_kz[j]; Zb[j] = W + o_zb[j]; }
    for (int l = 0; l <= N; ++l) a[l] = W + o_a[l];
    for (int l = 0; l < N; ++l) { d[l] = W + o_d[l]; v[l] = W + o_v[l]; acc2[l] = W + o_acc2[l]; dl[l] = W + o_dl[l]; }
    float* z[CNF_MAX_LAYERS];
    for (int l = 0; l < N; ++l) z[l] = o_z[l] >= 0 ? W + o_z[l] : nullptr;
    // where stage s (= step * ns + stage) keeps its activations: a[] / d[] (/ z[]) are pointed there before the stage's forward chain
    auto point_act = [&](long long stage) {
        float* q = W + o_actck + stage * act_stage;
        auto grab = [&](long long nfl) { float* r = q; q += (nfl + 63) / 64 * 64; return r; };
        a[0] = grab((long long)(c.widths[0] + 1) * B);
        for (int l = 0; l < N; ++l) {
            a[l + 1] = grab((long long)(L.wout[l] + 1) * B); d[l] = grab((long long)L.wout[l] * B);
            if (act_dd_needs_pre(L.act[l])) z[l] = grab((long long)L.wout[l] * B);
        }
    };
    float *lamv = W + o_lam, *kbar = W + o_kbar, *zs = W + o_zs, *gk = W + o_g, *gbar = W + o_gbar, *vN = W + o_vN;
    float *tdb = W + o_t0, *tdb2 = W + o_t1, *tvb = W + o_t2, *tsb = W + o_t3, *tab = W + o_t4;

    LG_HIP(zero_async(slabs, (size_t)npa_pad * nslab * sizeof(float), st));
    hipLaunchKernelGGL(aug_params_kernel, grid_for(npa), dim3(TPB), 0, st, P_dev, PA, L);

    ++G.epoch;   // PA was just rebuilt: operand images are repacked at their next use
    auto gemm = [&](int ta, int, int m, long long n, int k, const float* A, int lda, const float* Bm, int ldb, float* Cm,
                    int ldc) -> hipError_t {
        return lg_product(G, PA, ta, m, n, k, A, lda, Bm, ldb, Cm, ldc, LG_EPI_PLAIN, nullptr, 0, nullptr, 0, 0, st);
    };
    // Wbar_l[:, 0:ncols] += X Y^T, chunk by chunk into the slabs
    auto wgrad = [&](int l, const float* X, int ldx, const float* Y, int ldy, int ncols) -> hipError_t {
        return lg_wgrad(slabs + L.pa_off[l], npa_pad, kc, nslab, L.wout[l], ncols, X, ldx, Y, ldy, B, st);
    };
    // forward chain at (zs, t): a_l, act'_l for every layer (and z_l for swish / GELU); zdot = a_N
    auto forward = [&](const float* zin, float t) -> hipError_t {
        hipLaunchKernelGGL(build_input_kernel, grid_for((long long)(c.widths[0] + 1) * B), dim3(TPB), 0, st, zin, t, ys, a[0],
                           D, C, c.autonomous, B);
        for (int l = 0; l < N; ++l) {
            hipError_t s = lg_product(G, PA, OPN, L.wout[l], B, L.win[l] + 1, PA + L.pa_off[l], L.wout[l], a[l], L.win[l] + 1,
                                      a[l + 1], L.wout[l] + 1, LG_EPI_ACT, nullptr, 0, d[l], L.wout[l], L.act[l], st, nullptr,
                                      nullptr, 0, 0, z[l]);
            if (s != hipSuccess) return s;
        }
        return hipSuccess;
    };

    const Tableau T = make_tableau(alg);
    // step n runs from tgrid[n] to tgrid[n+1] when a grid is given (frozen steps of an adaptive solve), else uniform
    float dt = (t1 - t0) / (float)nsteps;
    auto step_t = [&](int n) { return tgrid ? tgrid[n] : t0 + (float)n * ((t1 - t0) / (float)nsteps); };
    auto step_dt = [&](int n) { return tgrid ? tgrid[n + 1] - tgrid[n] : (t1 - t0) / (float)nsteps; };
    const int ns = T.ns;
    int cur_step = 0;
    // stage derivatives of one step from z_n (z rows only: the gradient needs no trace here)
    auto stage_derivs = [&](const float* zn, float tn) -> hipError_t {
        for (int i = 0; i < ns; ++i) {
            Comb cb{};
            cb.nk = 0;
            for (int j = 0; j < i; ++j)
                if (T.a[i][j] != 0.f) { cb.k[cb.nk] = kz[j]; cb.coef[cb.nk] = dt * T.a[i][j]; ++cb.nk; }
            hipLaunchKernelGGL(combine_kernel, grid_for(DB), dim3(TPB), 0, st, zs, zn, cb, DB);
            if (keep_act) point_act((long long)cur_step * ns + i);
            hipError_t s = forward(zs, tn + T.c[i] * dt);
            if (s != hipSuccess) return s;
            hipLaunchKernelGGL(copy_rows_kernel, grid_for(DB), dim3(TPB), 0, st, kz[i], a[N], D, D + 1, 0, B);
        }
        return hipSuccess;
    };

    // ---- forward sweep: checkpoints z_n ----
    float* zck = W + o_zck;
    const float* cw = cot ? cot->u1_bar + D : nullptr;   // per-column cotangents of the dlogp / E / n rows (null: the shipped loss)
    const int ldw = D + 3;
    if (cot) hipLaunchKernelGGL(copy_rows_kernel, grid_for(DB), dim3(TPB), 0, st, zck, cot->u0, D, D + 3, 0, B);
    else hipLaunchKernelGGL(init_state_kernel, grid_for(DB), dim3(TPB), 0, st, x, zck, c.nvars, D, B);
    float* kck = W + o_kck;
    for (int n = 0; n < nsteps; ++n) {
        dt = step_dt(n);
        cur_step = n;
        LG_BLAS(stage_derivs(zck + (long long)n * DB, step_t(n)));
        if (keep_k)
            for (int j = 0; j < ns; ++j)
                LG_HIP(copy_async(kck + ((long long)n * ns + j) * DB, kz[j], (size_t)DB * sizeof(float), st));
        Comb cb{};
        cb.nk = ns;
        for (int j = 0; j < ns; ++j) { cb.k[j] = kz[j]; cb.coef[j] = dt * T.b[j]; }
        hipLaunchKernelGGL(combine_kernel, grid_for(DB), dim3(TPB), 0, st, zck + (long long)(n + 1) * DB, zck + (long long)n * DB, cb, DB);
    }
    if (cot) hipLaunchKernelGGL(copy_rows_kernel, grid_for(DB), dim3(TPB), 0, st, lamv, cot->u1_bar, D, D + 3, 0, B);
    else hipLaunchKernelGGL(lam_init_kernel, grid_for(B), dim3(TPB), 0, st, lamv, zck + (long long)nsteps * DB, lam[2], c.nvars, D, B);

    // ---- reverse sweep ----
    const float invK = exact ? 1.f : 1.f / (float)K;
    // the loss of this solve is accumulated on the way (no separate forward solve for it): per column dlogp, E, n
    // (the pullback of the solve: the same accumulators, started from u0's rows, are the dlogp / E / n rows of u1)
    const bool want_loss = cot ? cot->u1 != nullptr : (logp_out != nullptr && regs_out != nullptr);
    float *lacc = W + o_lacc, *eacc = lacc + B, *nacc = eacc + B;
    if (want_loss && cot) hipLaunchKernelGGL(cot_rows_init_kernel, grid_for(B), dim3(TPB), 0, st, lacc, eacc, nacc, cot->u0, D, B);
    else if (want_loss) LG_HIP(zero_async(lacc, 3 * (size_t)B * sizeof(float), st));
    const bool hutch = !exact;
    float* const ysum = W + o_ysum;
    if (ys_bar) LG_HIP(zero_async(ysum, (size_t)H1B * sizeof(float), st));
    int Gw = 1;                      // lanes per column of the grouped per-column kernels (0: D > 64, thread-per-column forms)
    while (Gw < D) Gw <<= 1;
    if (Gw > 64) Gw = 0;
    for (int n = nsteps - 1; n >= 0; --n) {
        const float* zn = zck + (long long)n * DB;
        dt = step_dt(n);
        const float tn = step_t(n);
        if (keep_k) { for (int j = 0; j < ns; ++j) kz[j] = kck + ((long long)n * ns + j) * DB; }
        else LG_BLAS(stage_derivs(zn, tn));
        for (int i = ns - 1; i >= 0; --i) {
            Comb cb{};
            cb.nk = 0;
            for (int j = 0; j < i; ++j)
                if (T.a[i][j] != 0.f) { cb.k[cb.nk] = kz[j]; cb.coef[cb.nk] = dt * T.a[i][j]; ++cb.nk; }
            if (keep_act) {
                point_act((long long)n * ns + i);      // a_l, act'_l of this stage as the forward sweep left them
            } else {
                hipLaunchKernelGGL(combine_kernel, grid_for(DB), dim3(TPB), 0, st, zs, zn, cb, DB);
                LG_BLAS(forward(zs, tn + T.c[i] * dt));
            }
            const float cl = dt * T.b[i];          // cotangent of ldot (dL/d dlogp = +1 per column)
            Comb zb{};
            zb.nk = 0;
            for (int j = i + 1; j < ns; ++j)
                if (T.a[j][i] != 0.f) { zb.k[zb.nk] = Zb[j]; zb.coef[zb.nk] = T.a[j][i]; ++zb.nk; }
            if (Gw) hipLaunchKernelGGL(kbar_grp_kernel, grid_for(B * Gw), dim3(TPB), 0, st, kbar, lamv, zb, dt * T.b[i], dt, a[N], cl * lam[0], D, Gw, B, cw, ldw);
            else hipLaunchKernelGGL(kbar_kernel, grid_for(B), dim3(TPB), 0, st, kbar, lamv, zb, dt * T.b[i], dt, a[N], cl * lam[0], D, B, cw, ldw);
            if (want_loss && hutch && c.reg_z) {
                if (Gw) hipLaunchKernelGGL(loss_acc_z_grp_kernel, grid_for(B * Gw), dim3(TPB), 0, st, eacc, a[N], D + 1, cl, D, Gw, B);
                else hipLaunchKernelGGL(loss_acc_z_kernel, grid_for(B), dim3(TPB), 0, st, eacc, a[N], D + 1, cl, D, B);
            }

            for (int k = 0; k < K; ++k) {
                if (exact) hipLaunchKernelGGL(onehot_kernel, grid_for(DB), dim3(TPB), 0, st, vN, k, D, B);
                else hipLaunchKernelGGL(copy_rows_kernel, grid_for(DB), dim3(TPB), 0, st, vN, eps, D, K * D, k * D, B);
                if (c.mode == CNF_MODE_HUTCH_JVP) {
                    // g = J eps_k by pushforward: r_l = W_l tau_{l-1} (tau_0 = eps on the z columns), tau_l = r_l .* act'_l;
                    // reverse: rbar_l = taubar_l .* act'_l, acc2_l += taubar_l .* r_l, Wbar_l += rbar_l tau_{l-1}^T,
                    // taubar_{l-1} = W_l^T rbar_l.  (r_l is kept in v[l], tau_l in dl[l].)
                    for (int l = 0; l < N; ++l) {
                        if (l == 0) LG_BLAS(gemm(OPN, OPN, L.wout[0], B, D, PA, L.wout[0], vN, D, v[0], L.wout[0]));
                        else LG_BLAS(gemm(OPN, OPN, L.wout[l], B, L.win[l], PA + L.pa_off[l], L.wout[l], dl[l - 1], L.win[l], v[l], L.wout[l]));
                        const long long HB = (long long)L.wout[l] * B;
                        hipLaunchKernelGGL(mul_kernel, grid_for(HB), dim3(TPB), 0, st, dl[l], v[l], d[l], HB);
                    }
                    if (Gw) {
                        hipLaunchKernelGGL(gbar_grp_kernel, grid_for(B * Gw), dim3(TPB), 0, st, gbar, dl[N - 1], vN, cl * invK, cl * lam[1] * invK,
                                           want_loss ? lacc : nullptr, nacc, -cl * invK, c.reg_j ? cl * invK : 0.f, D, Gw, B, cw, ldw);
                    } else {
                        hipLaunchKernelGGL(gbar_kernel, grid_for(B), dim3(TPB), 0, st, gbar, dl[N - 1], vN, cl * invK, cl * lam[1] * invK, D, B, cw, ldw);
                        if (want_loss)
                            hipLaunchKernelGGL(loss_acc_g_kernel, grid_for(B), dim3(TPB), 0, st, lacc, nacc, dl[N - 1], vN, -cl * invK,
                                               c.reg_j ? cl * invK : 0.f, D, B);
                    }
                    const float* tb = gbar;
                    float *tbn = tdb, *tbn2 = tdb2;
                    for (int l = N - 1; l >= 0; --l) {
                        const long long HB = (long long)L.wout[l] * B;
                        hipLaunchKernelGGL(bottom_kernel, grid_for(HB), dim3(TPB), 0, st, tb, d[l], v[l], tvb, acc2[l], k == 0 ? 1 : 0, HB);
                        if (l > 0) {
                            LG_BLAS(wgrad(l, tvb, L.wout[l], dl[l - 1], L.win[l], L.win[l]));
                            LG_BLAS(gemm(OPT, OPN, L.win[l], B, L.wout[l], PA + L.pa_off[l], L.wout[l], tvb, L.wout[l], tbn, L.win[l]));
                            tb = tbn;
                            float* tmp = tbn; tbn = tbn2; tbn2 = tmp;
                        } else {
                            LG_BLAS(wgrad(0, tvb, L.wout[0], vN, D, D));   // Wbar_1[:,0:D] += rbar_1 eps_k^T
                        }
                    }
                    continue;
                }
                // pullback of probe k: v_N = eps_k, delta_l = v_l .* act'_l, v_{l-1} = W_l^T delta_l, g = W_1[:,0:D]^T delta_1;
                // every product also writes delta_{l-1} = v_{l-1} .* act'_{l-1} (fused epilogue)
                hipLaunchKernelGGL(mul_kernel, grid_for(DB), dim3(TPB), 0, st, dl[N - 1], vN, d[N - 1], DB);
                for (int l = N - 1; l >= 1; --l)
                    LG_BLAS(lg_product(G, PA, OPT, L.win[l], B, L.wout[l], PA + L.pa_off[l], L.wout[l], dl[l], L.wout[l], v[l - 1], L.win[l],
                                       LG_EPI_MUL2, d[l - 1], L.win[l], dl[l - 1], L.win[l], 0, st));
                LG_BLAS(gemm(OPT, OPN, D, B, L.wout[0], PA, L.wout[0], dl[0], L.wout[0], gk, D));
                if (Gw) {
                    hipLaunchKernelGGL(gbar_grp_kernel, grid_for(B * Gw), dim3(TPB), 0, st, gbar, gk, vN, cl * invK, cl * lam[1] * invK,
                                       want_loss ? lacc : nullptr, nacc, -cl * invK, (hutch && c.reg_j) ? cl * invK : 0.f, D, Gw, B, cw, ldw);
                } else {
                    hipLaunchKernelGGL(gbar_kernel, grid_for(B), dim3(TPB), 0, st, gbar, gk, vN, cl * invK, cl * lam[1] * invK, D, B, cw, ldw);
                    if (want_loss)
                        hipLaunchKernelGGL(loss_acc_g_kernel, grid_for(B), dim3(TPB), 0, st, lacc, nacc, gk, vN, -cl * invK,
                                           (hutch && c.reg_j) ? cl * invK : 0.f, D, B);
                }
                // bottom-up through the pullback: dbar_1 = W_1[:,0:D] gbar, vbar_l = dbar_l .* act'_l, acc2_l += dbar_l .* v_l
                // (both in the epilogue of the product that makes dbar_l), dbar_{l+1} = W_{l+1} vbar_l
                float *cur = tvb, *nxt = tdb;
                LG_BLAS(lg_product(G, PA, OPN, L.wout[0], B, D, PA, L.wout[0], gbar, D, cur, L.wout[0], LG_EPI_BOTTOM, d[0], L.wout[0],
                                   acc2[0], L.wout[0], 0, st, N == 1 ? vN : v[0], nullptr, 0, k == 0 ? 1 : 0));
                LG_BLAS(wgrad(0, dl[0], L.wout[0], gbar, D, D));                                       // Wbar_1[:,0:D] += delta_1 gbar^T
                for (int l = 0; l + 1 < N; ++l) {
                    LG_BLAS(wgrad(l + 1, dl[l + 1], L.wout[l + 1], cur, L.wout[l], L.wout[l]));        // Wbar_{l+1} += delta_{l+1} vbar_l^T
                    LG_BLAS(lg_product(G, PA, OPN, L.wout[l + 1], B, L.wout[l], PA + L.pa_off[l + 1], L.wout[l + 1], cur, L.wout[l], nxt,
                                       L.wout[l + 1], LG_EPI_BOTTOM, d[l + 1], L.wout[l + 1], acc2[l + 1], L.wout[l + 1], 0, st,
                                       l + 1 == N - 1 ? vN : v[l + 1], nullptr, 0, k == 0 ? 1 : 0));
                    float* tmp = cur; cur = nxt; nxt = tmp;
                }
            }
            // top-down through the forward chain: sbar_l = abar_l .* act'_l + acc2_l .* act''_l (in the epilogue of the product
            // that makes abar_l), [Wbar_l | bbar_l] += sbar_l [a_{l-1}; 1]^T, abar_{l-1} = W_l^T sbar_l
            float *scur = tsb, *snxt = tab;
            // (act'' from a_l, or from z_l for swish / GELU)
            hipLaunchKernelGGL(sbar_kernel, grid_for((long long)L.wout[N - 1] * B), dim3(TPB), 0, st, scur, kbar, d[N - 1], acc2[N - 1],
                               z[N - 1] ? z[N - 1] : a[N], z[N - 1] ? L.wout[N - 1] : L.wout[N - 1] + 1, L.act[N - 1], L.wout[N - 1], B);
            for (int l = N - 1; l >= 0; --l) {
                LG_BLAS(wgrad(l, scur, L.wout[l], a[l], L.win[l] + 1, L.win[l] + 1));
                if (l > 0) {
                    LG_BLAS(lg_product(G, PA, OPT, L.win[l], B, L.wout[l], PA + L.pa_off[l], L.wout[l], scur, L.wout[l], snxt, L.win[l],
                                       LG_EPI_SBAR, d[l - 1], L.win[l], nullptr, 0, L.act[l - 1], st, acc2[l - 1],
                                       z[l - 1] ? z[l - 1] : a[l], z[l - 1] ? L.win[l] : L.win[l] + 1, 0));
                    float* tmp = scur; scur = snxt; snxt = tmp;
                } else {
                    LG_BLAS(gemm(OPT, OPN, D, B, L.wout[0], PA, L.wout[0], scur, L.wout[0], Zb[i], D));   // Zbar_i = W_1[:,0:D]^T sbar_1
                    if (ys_bar) {   // the conditions' share of sbar_1 is constant over the solve: summed here, multiplied once at the end
                        Comb cs{};
                        cs.nk = 1; cs.k[0] = scur; cs.coef[0] = 1.f;
                        hipLaunchKernelGGL(combine_kernel, grid_for(H1B), dim3(TPB), 0, st, ysum, ysum, cs, H1B);
                    }
                }
            }
        }
        Comb cb{};
        cb.nk = ns;
        for (int j = 0; j < ns; ++j) { cb.k[j] = Zb[j]; cb.coef[j] = 1.f; }
        hipLaunchKernelGGL(combine_kernel, grid_for(DB), dim3(TPB), 0, st, lamv, lamv, cb, DB);
    }
    hipLaunchKernelGGL(reduce_slabs_kernel, grid_for(npa), dim3(TPB), 0, st, slabs, nslab, npa_pad, L, grad);
    if (ys_bar)   // ys_bar = W_1[:, ycols]^T sum sbar_1 (the y columns follow z and, unless autonomous, the time column)
        LG_BLAS(gemm(OPT, OPN, C, B, L.wout[0], PA + (long long)L.wout[0] * (D + (c.autonomous ? 0 : 1)), L.wout[0], ysum, L.wout[0], ys_bar, C));
    if (cot) {
        if (cot->u0_bar) hipLaunchKernelGGL(cot_out_kernel, grid_for((long long)(D + 3) * B), dim3(TPB), 0, st, cot->u0_bar, lamv, cot->u1_bar, D, B);
        if (cot->u1) hipLaunchKernelGGL(pack_final_kernel, grid_for(B), dim3(TPB), 0, st, cot->u1, zck + (long long)nsteps * DB, lacc, eacc, nacc, D, B);
        LG_HIP(hipGetLastError());
        return hipSuccess;
    }
    if (grad_x)   // costate at t0: dL/dx = its first nvars rows
        hipLaunchKernelGGL(copy_rows_kernel, grid_for((long long)c.nvars * B), dim3(TPB), 0, st, grad_x, lamv, c.nvars, D, 0, B);
    if (want_loss) {   // inference_sol on [z(t1); dlogp; E; n] (src/core/base_icnf.jl:158-172)
        float* ufin = W + o_ufin;
        hipLaunchKernelGGL(pack_final_kernel, grid_for(B), dim3(TPB), 0, st, ufin, zck + (long long)nsteps * DB, lacc, eacc, nacc, D, B);
        const int ra = (hutch && c.reg_aug && c.naug > 0) ? 1 : 0;
        LG_HIP(epilogue(ufin, c.nvars, D, ra, B, logp_out, regs_out, st));
    }
    LG_HIP(hipGetLastError());
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------------------------
// Cooperative gradient for wide hidden layers (cnf_coop_grad.hip): checkpointing forward solve, one reverse-sweep launch
// per RK step, then one weight-cotangent product per weight matrix per step over the operands that launch left
// ---------------------------------------------------------------------------------------------------------------------
// dst[e] += sum of the n slabs src[c * sz + e], fixed order (the D-row cotangent's own, finer chunking folded into slab 0)
__global__ void fold_slabs_kernel(float* __restrict__ dst, const float* __restrict__ src, int n, long long sz) {
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= sz) return;
    // eight independent partial sums (slabs c = k mod 8) keep eight loads in flight; combined in a fixed order
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int c = 0;
    for (; c + 8 <= n; c += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += src[(long long)(c + k) * sz + e];
    }
    for (int k = 0; c < n; ++c, ++k) acc[k] += src[(long long)c * sz + e];
    dst[e] += ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// rows [row0, rows) of columns [c0, c1) of a column-major array <- val
__global__ void fill_rows_kernel(float* __restrict__ a, int ld, int row0, int rows, long long c0, long long c1, float val) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    const int nr = rows - row0;
    if (i >= (c1 - c0) * nr) return;
    a[(c0 + i / nr) * ld + row0 + (int)(i % nr)] = val;
}

// The sweep kernel addresses its operand arrays through 32-bit buffer resources and 32-bit byte offsets: the largest array
// ((H + 1, padded) rows x 2 x stages x B columns of floats) has to stay below 2 GB.  Larger batches take the layer-wise path.
long long coop_grad_max_columns(const cnf_config& c, int alg) {
    const long long ldy = (c.widths[1] + 1 + 15) / 16 * 16, ns = make_tableau(alg).ns;
    return 0x7fffffffLL / (ldy * 4 * 2 * ns);
}

bool coop_grad_eligible(const cnf_config& c, const MfmaPlan* plan, const float lam[3], bool on_grid) {
    int HT, L, ZR, ACT, CR;
    if (!mfma_plan_coop_grad_shape(plan, &HT, &L, &ZR, &ACT, &CR)) return false;
    if (tuning().coop_grad == 0) return false;
    if (c.mode != CNF_MODE_HUTCH_VJP || c.nprobes != 1 || (c.ncond != 0) != (CR != 0)) return false;
    // the forward solve must be able to checkpoint: on a non-uniform grid (the frozen steps of an adaptive solve) a cooperative
    // plan does so through the extended kernel's instance of exactly its own layout, if there is one
    if (!mfma_plan_can_checkpoint(plan, on_grid)) return false;
    if (c.n_layers != L + 1) return false;
    for (int l = 0; l < L; ++l)
        if ((c.acts[l] != CNF_ACT_TANH && c.acts[l] != CNF_ACT_SOFTPLUS) || c.acts[l] != c.acts[0] || c.widths[l + 1] != c.widths[1]) return false;
    if (c.acts[L] != CNF_ACT_IDENTITY) return false;
    if (c.widths[1] % 4 != 0) return false;                   // 16-byte row quads of the operand arrays
    return coop_grad_supported(HT, L, ZR, CR, ACT) && lg_wgrad_supported(c.widths[1], c.widths[1] + 1);
}


// ---------------------------------------------------------------------------------------------------------------------
// The cooperative gradient in its SECOND FORM (round 6): the checkpointing forward solve also stores h_l
// and delta_l of every stage (tile-native, cnf_tiles.h), the sweep (cnf_coop_grad3.hip) runs the second-order chains alone
// and leaves vbar_l / sbar_l as tiles, and the weight cotangents are products over tiles (cnf_wgrad_tiles.hip) whose other
// operands are the forward solve's store.  Same checkpoints, same costate algebra, same slabs and final reduction as coop_grad.
// ---------------------------------------------------------------------------------------------------------------------
static bool coop_grad3_fits(const cnf_config& c, int HTs, int Lh, int alg, int nsteps, long long ntp) {
    const long long ns = make_tableau(alg).ns;
    StageStore S{Lh, nsteps, (int)ns, HTs, ntp};
    const long long gib = tuning().coop_grad3_gib > 0 ? tuning().coop_grad3_gib : 0;
    if (S.total() * 4 > (gib << 30)) return false;
    const int D = c.nvars + c.naug;
    const long long dtz = (c.widths[0] + 15) / 16 > (D + 15) / 16 ? (c.widths[0] + 15) / 16 : (D + 15) / 16;
    // the sweep addresses a step's arrays through 32-bit byte offsets
    return ns * ntp * (HTs > dtz ? HTs : dtz) * 1024 < 0x7fffffffLL;
}

// Does a cooperative gradient call of B columns, `nsteps` steps of `alg`, take the second form - and with how many hidden tiles per
// sample tile in its stage store (0: no, the recomputing sweeps serve it)?  Uniform steps only; the sweep must have an instance
// for the shape, the forward solve's kernel must write the store, and HBM must have room for it (CNF_COOP_GRAD3_GIB).
int coop_grad_stage_store_tiles(const cnf_config& c, MfmaPlan* plan, long long B, int alg, int nsteps, bool on_grid) {
    int HT, Lh, ZR, ACT, CR;
    if (on_grid || tuning().coop_grad3 == 0 || nsteps < 1 || !mfma_plan_coop_grad_shape(plan, &HT, &Lh, &ZR, &ACT, &CR) || CR != 0) return 0;
    if (!coop_grad3_supported(c.widths[1], c.nvars + c.naug, Lh, ACT, HT, ZR, CR)) return 0;
    const int HTs = mfma_plan_stage_store_tiles(plan, B, false);
    if (HTs <= 0 || !coop_grad3_fits(c, HTs, Lh, alg, nsteps, mfma_plan_ckpt_tiles(plan, B, false))) return 0;
    return HTs;
}

static hipError_t coop_grad3_run(LayeredGrad& G, const cnf_config& c, MfmaPlan* plan, const float* packed_dev, const size_t* w_off, const size_t* b_off,
                                 const float* x, const float* eps, const float* ys, int alg, int nsteps, float t0, float t1, long long B, const float lam[3],
                                 float* grad, float* grad_x, float* logp_out, float* regs_out, int HT, int Lh, int ZR, int ACT, int HTs, hipStream_t st, std::string* err) {
    const int D = c.nvars + c.naug, H = c.widths[1], n_in = c.widths[0];
    const LDesc L = make_ldesc(c, w_off, b_off);
    const long long npa = L.npa;
    const long long npa_pad = (npa + 63) / 64 * 64;
    const Tableau T = make_tableau(alg);
    const int ns = T.ns;
    const long long ntp = mfma_plan_ckpt_tiles(plan, B, false);
    const long long nct = (long long)ns * ntp;              // column tiles of a step
    const int DT = (D + 15) / 16, DTZ = (n_in + 15) / 16 > DT ? (n_in + 15) / 16 : DT;
    // chunks (= slabs) of the three kinds of product
    long long ch1 = 0, chH = 0, chN = 0;
    const int nc1 = wgrad_tiles_chunks(H, n_in, nct, G.num_cus, &ch1), ncH = wgrad_tiles_chunks(H, H, nct, G.num_cus, &chH),
              ncN = wgrad_tiles_chunks(D, H, nct, G.num_cus, &chN);
    const int nslab = std::max(nc1, std::max(ncH, ncN));
    StageStore S{Lh, nsteps, ns, HTs, ntp};
    LG_HIP(G.ws_store.reserve((size_t)S.total()));
    Carver take;
    const long long o_slab = take(npa_pad * nslab);
    const long long o_zck = take((long long)(nsteps + 1) * ntp * 64 * ZR), o_kck = take((long long)nsteps * ns * ntp * 64 * ZR);
    const long long o_gck = lam[1] != 0.f ? take((long long)nsteps * ns * ntp * 64 * ZR) : 0;
    const int KZ = (ZR + 3) / 4 * 4;
    const long long o_lam = take(ntp * 64 * KZ), o_zb = take(ntp * 64 * 6 * KZ);
    long long o_sv[3], o_ss[3];
    for (int l = 0; l < Lh; ++l) { o_sv[l] = take(nct * HTs * 256); o_ss[l] = take(nct * HTs * 256); }
    const long long o_gb = take(nct * DTZ * 256), o_zt = take(nct * DTZ * 256), o_ep = take(nct * DT * 256), o_kb = take(nct * DT * 256);
    LG_HIP(G.ws.reserve((size_t)take.off));
    float* W = G.ws;
    float* slabs = W + o_slab;
    LG_HIP(zero_async(slabs, (size_t)npa_pad * nslab * sizeof(float), st));

    // ---- forward: the cooperative solve, checkpointing z_n and the stage derivatives AND storing h_l / delta_l of every stage ----
    SolveArgs sa{};
    sa.x = x; sa.eps = eps; sa.ys = ys; sa.B = B; sa.nsteps = nsteps; sa.alg = alg; sa.t0 = t0; sa.t1 = t1;
    sa.logp = logp_out; sa.regs = regs_out; sa.nvars = c.nvars; sa.reg_aug = (c.reg_aug && c.naug > 0) ? 1 : 0;
    sa.ckpt = W + o_zck; sa.ckpt_k = W + o_kck; sa.ckpt_g = lam[1] != 0.f ? W + o_gck : nullptr;
    sa.kfull = G.ws_store;
    // two hidden layers: the sweep with two workgroups per CU (cnf_coop_grad3w.hip) once there are more 32-sample super-tiles than CUs - with
    // one workgroup per CU anyway the one-per-CU sweep, which requests a stage ahead, is the faster of the two (0.51 against 0.55 ms per
    // launch at nvariables = 20); the two agree bit for bit, so the choice moves no number.  CNF_COOP_GRAD3=2 keeps the one-per-CU sweep, =3
    // takes the two-per-CU one at every size (A/B, tests)
    const int g3sw = tuning().coop_grad3;
    const bool paired = g3sw != 2 && (g3sw == 3 || ntp / 2 > G.num_cus) && coop_grad3w_supported(H, D, Lh, ACT, HT, ZR, 0);
    // the checkpoint rows as tiles where the forward solve's kernel writes that layout (the dealt 64-sample form) and the two-per-CU sweep
    // reads them: up to 12 state registers - D <= 48 - a sweep reads three of a lane's four 16-byte groups and the layout pays (nvariables =
    // 20: 48.8 -> 47.7 ms); with 16 every line is used either way
    const bool ck_tiles = paired && D <= 48 && mfma_plan_ckpt_rows_as_tiles(plan, B, false);
    sa.ck_tiles = ck_tiles ? 1 : 0;
    LG_HIP(mfma_solve(plan, packed_dev, sa, st));

    // ---- reverse: one sweep launch per step, then the step's weight-cotangent products over tiles ----
    CG3Args a{};
    a.c.packed = packed_dev; a.c.eps = eps; a.c.ys = ys; a.c.C = 0; a.c.ckpt = W + o_zck; a.c.ckpt_k = W + o_kck; a.c.ckpt_g = sa.ckpt_g;
    a.c.lam = W + o_lam; a.c.zb = W + o_zb; a.c.grad_x = grad_x;
    a.c.B = B; a.c.ntiles_pad = ntp; a.c.nsteps = nsteps; a.c.D = D; a.c.nvars = c.nvars; a.c.H = H; a.c.autonomous = c.autonomous;
    a.c.lam1 = lam[0]; a.c.lam2 = lam[1]; a.c.lam3 = lam[2]; a.c.T = T;
    for (int l = 0; l < Lh; ++l) { a.sv[l] = W + o_sv[l]; a.ss[l] = W + o_ss[l]; }
    a.gb = W + o_gb; a.zt = W + o_zt; a.ep = W + o_ep; a.kb = W + o_kb;
    a.HTs = HTs; a.DTZ = DTZ; a.DTs = DT; a.ck_tiles = ck_tiles ? 1 : 0;
    const float dt = (t1 - t0) / (float)nsteps;
    // (Tried, round 6: the three kinds of product of a step - disjoint slab regions, disjoint operands; the D-sized ones bound by
    // reading their H-row operand once, the H x H ones by the matrix pipe - side by side on three library-owned streams, joined
    // before the next sweep: cfg4 86.4 -> 88.7 ms, default architecture nv = 20 / 28 52.2 -> 53.9 / 83.6 -> 86.9 ms.  Concurrent
    // kernels slow each other down by more than the overlap gains, as round 3 found for the older form.  Also tried: the two D-sized
    // products (bound by reading their H-row operand once) on a second stream beside the NEXT step's sweep, launched on 8 / 16 / 32
    // fewer CUs, their inputs double-buffered: cfg4 85.7 -> 93.3 ms (1024 super-tiles on 240 workgroups are five rounds, not four),
    // nv = 20 50.9 -> 51.4.  One stream.)
    for (int n = nsteps - 1; n >= 0; --n) {
        a.c.step = n; a.c.tn = t0 + (float)n * dt; a.c.dt = dt;
        for (int l = 0; l < Lh; ++l) { a.fh[l] = G.ws_store + S.at(0, l, n, 0); a.fd[l] = G.ws_store + S.at(1, l, n, 0); }
        if (paired) LG_HIP(coop_grad3w_step_launch(H, D, Lh, ACT, HT, ZR, a, G.num_cus, st));
        else LG_HIP(coop_grad3_step_launch(H, D, Lh, ACT, HT, ZR, a, G.num_cus, st));
        // Wbar_{l+1} += delta_{l+1} vbar_l^T + sbar_{l+1} h_l^T
        for (int l = 1; l < Lh; ++l)
            LG_HIP(wgrad_tiles(slabs + L.pa_off[l], npa_pad, chH, ncH, H, H, WTTerm{a.fd[l], a.sv[l - 1], HTs, HTs}, WTTerm{a.ss[l], a.fh[l - 1], HTs, HTs}, nct, 1, st));
        // Wbar_1 += delta_1 gbar^T + sbar_1 [z; t]^T  (bias: row sums of sbar_1)
        LG_HIP(wgrad_tiles(slabs + L.pa_off[0], npa_pad, ch1, nc1, H, n_in, WTTerm{a.fd[0], a.gb, HTs, DTZ}, WTTerm{a.ss[0], a.zt, HTs, DTZ}, nct, 1, st));
        // Wbar_N += eps cbar^T + kbar h_L^T  (bias: row sums of kbar)
        LG_HIP(wgrad_tiles(slabs + L.pa_off[Lh], npa_pad, chN, ncN, D, H, WTTerm{a.ep, a.sv[Lh - 1], DT, HTs}, WTTerm{a.kb, a.fh[Lh - 1], DT, HTs}, nct, 1, st));
    }
    hipLaunchKernelGGL(reduce_slabs_kernel, grid_for(npa), dim3(TPB), 0, st, slabs, nslab, npa_pad, L, grad);
    LG_HIP(hipGetLastError());
    (void)err;
    return hipSuccess;
}

hipError_t coop_grad(LayeredGrad** ctx, const cnf_config& c, MfmaPlan* plan, const float* packed_dev, const size_t* w_off,
                     const size_t* b_off, const float* x, const float* eps, const float* ys, int alg, int nsteps, float t0, float t1,
                     const float* tgrid, const float* tgrid_dev, long long B, const float lam[3], float* grad, float* grad_x, float* logp_out, float* regs_out, hipStream_t st, std::string* err) {
    int HT, Lh, ZR, ACT, CR;
    if (!mfma_plan_coop_grad_shape(plan, &HT, &Lh, &ZR, &ACT, &CR)) { *err = "coop_grad: not a cooperative plan"; return hipErrorNotSupported; }
    if (!*ctx) *ctx = new LayeredGrad();
    LayeredGrad& G = **ctx;
    if (hipError_t e = lg_num_cus(G, err)) return e;
    if (const int HTs = coop_grad_stage_store_tiles(c, plan, B, alg, nsteps, tgrid != nullptr))
        return coop_grad3_run(G, c, plan, packed_dev, w_off, b_off, x, eps, ys, alg, nsteps, t0, t1, B, lam, grad, grad_x, logp_out, regs_out, HT, Lh, ZR, ACT, HTs, st, err);
    const int D = c.nvars + c.naug, H = c.widths[1], n_in = c.widths[0];
    const LDesc L = make_ldesc(c, w_off, b_off);
    const long long npa = L.npa;
    const long long npa_pad = (npa + 63) / 64 * 64;
    const Tableau T = make_tableau(alg);
    const int ns = T.ns;
    const long long B2 = 2LL * ns * B;                      // columns of every operand array
    long long kc = 0;
    const int nslab = lg_wgrad_chunks(H, B2, G.num_cus, &kc, 4);
    // The D-row cotangent (Wbar_N = [eps | kbar] Y_L^T: D x (H + 1)) is one row block: with the square layers' chunking it would
    // run on a quarter of their workgroups (one per CU: 127 us for 270 MB).  It gets its own, finer chunks and slabs.
    long long kcN = 0;
    const int nslabN = lg_wgrad_chunks(D, B2, G.num_cus, &kcN, 4, H + 1);
    const long long szN = (long long)D * (H + 1), szN_pad = (szN + 63) / 64 * 64;
    const long long ntp = mfma_plan_ckpt_tiles(plan, B, tgrid != nullptr);
    const int cg_nt = coop_grad_nt(HT, Lh, ZR, CR, ACT);   // sample tiles per super-tile of the sweep instance
    const int nblocks = coop_grad_nblocks(B, G.num_cus, HT, ZR, CR, cg_nt);
    const int slots = coop_grad_scratch_slots(Lh);
    const long long scratch_stride = (long long)(slots > 0 ? slots : 1) * HT * 256 * cg_nt;   // slots x (HT tiles x NT sample tiles x 64 lanes x 4) floats

    Carver take;
    const long long o_slab = take(npa_pad * nslab), o_slabN = take(szN_pad * nslabN);
    const long long o_zck = take((long long)(nsteps + 1) * ntp * 64 * ZR), o_kck = take((long long)nsteps * ns * ntp * 64 * ZR);
    const long long o_gck = lam[1] != 0.f ? take((long long)nsteps * ns * ntp * 64 * ZR) : 0;
    const long long o_lam = take(ntp * 64 * ZR), o_zb = take(ntp * 64 * 6 * ZR), o_scr = take(scratch_stride * nblocks);
    // Y_l: H + 1 rows; a leading dimension that is a multiple of 16 floats keeps every 16-byte operand store inside one
    // 64-byte block (H + 1 itself puts 15 of 16 samples' row quads across two)
    const int ldy = (H + 1 + 15) / 16 * 16;
    long long o_xh[3], o_yh[3];
    for (int l = 0; l < Lh; ++l) { o_xh[l] = take((long long)H * B2); o_yh[l] = take((long long)ldy * B2); }
    const long long o_y1 = take((long long)(n_in + 1) * B2), o_xN = take((long long)D * B2);
    LG_HIP(G.ws.reserve((size_t)take.off));
    float* W = G.ws;
    float* slabs = W + o_slab;
    LG_HIP(zero_async(slabs, (size_t)npa_pad * nslab * sizeof(float), st));
    LG_HIP(zero_async(W + o_slabN, (size_t)szN_pad * nslabN * sizeof(float), st));
    // constant rows of the operand arrays: the zero / ones row of every Y_l, the zero rows under gbar
    LG_HIP(zero_async(W + o_y1, (size_t)(n_in + 1) * B2 * sizeof(float), st));
    for (int l = 0; l < Lh; ++l) {
        hipLaunchKernelGGL(fill_rows_kernel, grid_for((long long)ns * B), dim3(TPB), 0, st, W + o_yh[l], ldy, H, H + 1, 0LL, (long long)ns * B, 0.f);
        hipLaunchKernelGGL(fill_rows_kernel, grid_for((long long)ns * B), dim3(TPB), 0, st, W + o_yh[l], ldy, H, H + 1, (long long)ns * B, B2, 1.f);
    }

    // ---- forward: the cooperative solve, checkpointing z_n and the stage derivatives; it also delivers the loss terms ----
    SolveArgs sa{};
    sa.x = x; sa.eps = eps; sa.ys = ys; sa.B = B; sa.nsteps = nsteps; sa.alg = alg; sa.t0 = t0; sa.t1 = t1;
    sa.logp = logp_out; sa.regs = regs_out; sa.nvars = c.nvars; sa.reg_aug = (c.reg_aug && c.naug > 0) ? 1 : 0;
    sa.ckpt = W + o_zck; sa.ckpt_k = W + o_kck; sa.ckpt_g = lam[1] != 0.f ? W + o_gck : nullptr;
    sa.tgrid_dev = tgrid ? tgrid_dev : nullptr;
    LG_HIP(mfma_solve(plan, packed_dev, sa, st));

    // ---- reverse: one launch per step, then the step's weight-cotangent products ----
    // (The products of step n on a second stream under the sweep of step n - 1, operand arrays double-buffered, was measured:
    // cfg4 117 -> 131 ms.  Both kernels are bound by memory traffic and slow each other down by more than the overlap gains.)
    CGArgs a{};
    a.packed = packed_dev; a.eps = eps; a.ys = ys; a.C = c.ncond; a.ckpt = W + o_zck; a.ckpt_k = W + o_kck; a.ckpt_g = sa.ckpt_g; a.lam = W + o_lam; a.zb = W + o_zb; a.grad_x = grad_x;
    a.scratch = W + o_scr; a.scratch_stride = scratch_stride;
    for (int l = 0; l < Lh; ++l) { a.xh[l] = W + o_xh[l]; a.yh[l] = W + o_yh[l]; }
    a.y1 = W + o_y1; a.xN = W + o_xN; a.ld_y1 = n_in + 1; a.ldy = ldy;
    a.B = B; a.ntiles_pad = ntp; a.nsteps = nsteps; a.D = D; a.nvars = c.nvars; a.H = H; a.autonomous = c.autonomous; a.lam1 = lam[0]; a.lam2 = lam[1]; a.lam3 = lam[2]; a.T = T;
    const bool dealt = coopd_grad_supported(H, D, Lh, ACT, HT, ZR, CR);   // the dealt sweep (cnf_coop_dgrad.hip) where it has an instance
    const float dt = (t1 - t0) / (float)nsteps;
    for (int n = nsteps - 1; n >= 0; --n) {
        a.step = n; a.tn = t0 + (float)n * dt; a.dt = dt;
        if (tgrid) { a.tn = tgrid[n]; a.dt = tgrid[n + 1] - tgrid[n]; }
        if (dealt) LG_HIP(coopd_grad_step_launch(H, D, Lh, ACT, HT, ZR, a, G.num_cus, st));
        else LG_HIP(coop_grad_step_launch(HT, Lh, ZR, CR, ACT, a, G.num_cus, st));
        LG_HIP(lg_wgrad(slabs + L.pa_off[0], npa_pad, kc, nslab, H, n_in + 1, a.xh[0], H, a.y1, n_in + 1, B2, st));
        for (int l = 1; l < Lh; ++l)
            LG_HIP(lg_wgrad(slabs + L.pa_off[l], npa_pad, kc, nslab, H, H + 1, a.xh[l], H, a.yh[l - 1], ldy, B2, st));
        LG_HIP(lg_wgrad(W + o_slabN, szN_pad, kcN, nslabN, D, H + 1, a.xN, D, a.yh[Lh - 1], ldy, B2, st));
    }
    hipLaunchKernelGGL(fold_slabs_kernel, grid_for(szN), dim3(TPB), 0, st, slabs + L.pa_off[Lh], W + o_slabN, nslabN, szN_pad);
    hipLaunchKernelGGL(reduce_slabs_kernel, grid_for(npa), dim3(TPB), 0, st, slabs, nslab, npa_pad, L, grad);
    LG_HIP(hipGetLastError());
    return hipSuccess;
}

}  // namespace cnf
