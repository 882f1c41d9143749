// cnf_common.h — shared host/device definitions for libcnf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "cnf.h"

namespace cnf {

// ---------------------------------------------------------------------------------------
// Fixed-step explicit Runge-Kutta tableaux, rounded to float (OrdinaryDiffEq converts its
// tableau to T = Float32).  Values: SURVEY.md §8 A4 (Tsitouras 2011); classic RK4.
// ---------------------------------------------------------------------------------------
// One table of decimal literals serves both precisions: TableauT<float> = Tableau (what the f32 kernels have always received:
// every literal rounded once to float) and TableauT<double> = TableauD for the double-precision path (cnf_f64.hip), whose
// coefficients never pass through float.
template <class Real>
struct TableauT {
    int ns;          // stage evaluations per step
    Real c[6];
    Real a[6][6];    // a[i][j], j < i
    Real b[6];
};
using Tableau = TableauT<float>;
using TableauD = TableauT<double>;

template <class Real>
inline TableauT<Real> make_tableau_as(int alg) {
    TableauT<Real> T{};
    auto r = [](double v) { return (Real)v; };
    if (alg == CNF_ALG_RK4) {
        T.ns = 4;
        const Real c[4] = {r(0.0), r(0.5), r(0.5), r(1.0)};
        const Real b[4] = {r(1.0) / r(6.0), r(1.0) / r(3.0), r(1.0) / r(3.0), r(1.0) / r(6.0)};
        for (int i = 0; i < 4; ++i) { T.c[i] = c[i]; T.b[i] = b[i]; }
        T.a[1][0] = r(0.5);
        T.a[2][1] = r(0.5);
        T.a[3][2] = r(1.0);
    } else {
        T.ns = 6;
        const Real c[6] = {r(0.0), r(0.161), r(0.327), r(0.9), r(0.9800255409045097), r(1.0)};
        const Real b[6] = {r(0.09646076681806523), r(0.01), r(0.4798896504144996),
                           r(1.379008574103742), r(-3.290069515436081), r(2.324710524099774)};
        for (int i = 0; i < 6; ++i) { T.c[i] = c[i]; T.b[i] = b[i]; }
        T.a[1][0] = r(0.161);
        T.a[2][0] = r(-0.008480655492356989); T.a[2][1] = r(0.335480655492357);
        T.a[3][0] = r(2.8971530571054935);    T.a[3][1] = r(-6.359448489975075);
        T.a[3][2] = r(4.3622954328695815);
        T.a[4][0] = r(5.325864828439257);     T.a[4][1] = r(-11.748883564062828);
        T.a[4][2] = r(7.4955393428898365);    T.a[4][3] = r(-0.09249506636175525);
        T.a[5][0] = r(5.86145544294642);      T.a[5][1] = r(-12.92096931784711);
        T.a[5][2] = r(8.159367898576159);     T.a[5][3] = r(-0.071584973281401);
        T.a[5][4] = r(-0.028269050394068383);
    }
    return T;
}
inline Tableau make_tableau(int alg) { return make_tableau_as<float>(alg); }
inline TableauD make_tableau_f64(int alg) { return make_tableau_as<double>(alg); }

// ---------------------------------------------------------------------------------------
// Activations.  act_fwd returns h = act(a) and writes d = act'(a).
//   tanh     : h = 2/(1+exp(-2a)) - 1;  d = 1 - h^2
//   softplus : NNlib.softplus(a) = log1p(exp(-|a|)) + relu(a);  d = sigmoid(a)
// Built from v_exp_f32 / v_log_f32 / v_rcp_f32 (about 1 ulp each); absolute error of h and d
// is <= 2e-7, checked against the fp64 oracle in tests/test_parity_gpu.py.
// The layer-wise and SIMT paths also take sigmoid, swish, ELU and GELU (act_fwd_rt below); the fused
// kernels are instantiated for tanh and softplus only.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
// v_sqrt_f32 alone (1 ulp; a denormal argument gives 0): sqrtf expands to a scaled, Newton-corrected sequence of ~12 VALU
// instructions, and the RNODE regularisers take K + 1 square roots per dynamics call
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// internal: tanh whose pre-activation arrives already multiplied by -2 log2(e) (the factor is folded
// into the forward weight images and biases by mfma_pack), so exp(-2a) is a bare v_exp_f32
constexpr int CNF_ACT_TANH_PRESCALED = 3;
constexpr float kTanhPrescale = -2.8853900817779268f;

template <int ACT>
__device__ __forceinline__ float act_fwd(float a, float& d) {
    if constexpr (ACT == CNF_ACT_TANH_PRESCALED) {
        const float e = __builtin_amdgcn_exp2f(a);
        const float r = fast_rcp(1.f + e);
        const float h = fmaf(2.f, r, -1.f);
        d = fmaf(-h, h, 1.f);
        return h;
    } else if constexpr (ACT == CNF_ACT_TANH) {
        // tanh(a) = 2 sigmoid(2a) - 1: one v_mul, v_exp, v_add, v_rcp, two v_fma.  Saturates
        // correctly (e -> inf gives r = 0, h = -1; e -> 0 gives h = 1); |error| <= 2e-7.
        const float e = __builtin_amdgcn_exp2f(a * -2.8853900817779268f);   // exp(-2a)
        const float r = fast_rcp(1.f + e);
        const float h = fmaf(2.f, r, -1.f);
        d = fmaf(-h, h, 1.f);
        return h;
    } else if constexpr (ACT == CNF_ACT_SOFTPLUS) {
        const float e = fast_exp(-fabsf(a));          // in (0,1]
        const float r = fast_rcp(1.f + e);
        d = a >= 0.f ? r : e * r;                     // sigmoid(a)
        return __logf(1.f + e) + fmaxf(a, 0.f);
    } else {
        d = 1.f;
        return a;
    }
}

// sigmoid(x) and 1 - sigmoid(x) from e = exp(-|x|) in (0, 1]: neither overflows, and the smaller of the two keeps its
// relative accuracy (1 - s is not formed by cancellation)
__device__ __forceinline__ void sigmoid_pair(float x, float& s, float& c) {
    const float e = fast_exp(-fabsf(x));
    const float r = fast_rcp(1.f + e);
    const float p = e * r;
    s = x >= 0.f ? r : p;
    c = x >= 0.f ? p : r;
}
constexpr float kGeluK0 = 0.7978845608028654f;    // sqrt(2 / pi)
constexpr float kGeluK1 = 0.035677408136300125f;  // sqrt(2 / pi) * 0.044715
// a with |a| clamped to 1e4 (a NaN passes through): past |a| ~ 10, sigmoid(2u) is exactly 0 or 1, so nothing but the overflow changes
__device__ __forceinline__ float gelu_tail(float a) { return fabsf(a) > 1e4f ? copysignf(1e4f, a) : a; }

// sigmoid : h = s = 1/(1+exp(-a));            d = s (1 - s)
// swish   : h = a s;                          d = s + h (1 - s)                     (NNlib.swish, SiLU)
// ELU     : h = a (a >= 0), exp(a) - 1;       d = 1 (a >= 0), exp(a)                (NNlib.elu, alpha = 1)
// GELU    : h = a sigmoid(2u), u = sqrt(2/pi) (a + 0.044715 a^3) = a/2 (1 + tanh u);
//           d = s + 2 a s (1 - s) u'                                                 (NNlib.gelu, tanh form)
// Every form, act_dd_rt below included, is free of NaN for every finite a: exp only ever sees a non-positive argument, and the
// products that meet a large |a| meet an s (1 - s) that underflows to 0 first (swish at a = -90 gives h = -0).  GELU's u' and
// a u'^2 would overflow first (a u'^2 near |a| ~ 1e8): their a is clamped to +-1e4 (gelu_tail), where s (1 - s) is already 0.
// identity / tanh / softplus: the activations of the fused kernels (the layer-wise instances built for them run this)
__device__ __forceinline__ float act_fwd_rt3(int act, float a, float& d) {
    if (act == CNF_ACT_TANH) return act_fwd<CNF_ACT_TANH>(a, d);
    if (act == CNF_ACT_SOFTPLUS) return act_fwd<CNF_ACT_SOFTPLUS>(a, d);
    d = 1.f;
    return a;
}

// every id of cnf.h
__device__ __forceinline__ float act_fwd_rt(int act, float a, float& d) {
    if (act == CNF_ACT_SIGMOID) {
        float s, c;
        sigmoid_pair(a, s, c);
        d = s * c;
        return s;
    }
    if (act == CNF_ACT_SWISH) {
        float s, c;
        sigmoid_pair(a, s, c);
        const float h = a * s;
        d = fmaf(h, c, s);
        return h;
    }
    if (act == CNF_ACT_ELU) {
        const float e = fast_exp(fminf(a, 0.f));
        // exp(a) - 1 cancels near 0: the cubic Taylor form below |a| = 2^-5 (error < a^4 / 24 = 4e-8), so h < 0 for every a < 0
        const float em1 = fabsf(a) < 0.03125f ? a * fmaf(a, fmaf(a, 0.16666667f, 0.5f), 1.f) : e - 1.f;
        d = a >= 0.f ? 1.f : e;
        return a >= 0.f ? a : em1;
    }
    if (act == CNF_ACT_GELU) {
        const float t = gelu_tail(a), t2 = t * t;
        float s, c;
        sigmoid_pair(2.f * t * fmaf(kGeluK1, t2, kGeluK0), s, c);
        const float du = fmaf(3.f * kGeluK1, t2, kGeluK0);          // u'
        d = fmaf(2.f * t * s * c, du, s);
        return a * s;
    }
    return act_fwd_rt3(act, a, d);
}

// act''(a) of every activation id, from x and d = act'(a): x is h = act(a) for tanh, sigmoid and ELU, the pre-activation a for
// swish and GELU (act_dd_needs_pre: their act'' is not a function of (h, act')), unused for identity and softplus.
// An id outside the enum gives NaN, never a silent 0 (the host checks the ids before every launch as well).
__host__ __device__ constexpr bool act_dd_needs_pre(int act) { return act == CNF_ACT_SWISH || act == CNF_ACT_GELU; }
__host__ __device__ constexpr bool act_dd_reads_x(int act) {
    return act == CNF_ACT_TANH || act == CNF_ACT_SIGMOID || act == CNF_ACT_ELU || act_dd_needs_pre(act);
}
__host__ __device__ constexpr bool act_id_valid(int act) {
    return act == CNF_ACT_IDENTITY || act == CNF_ACT_TANH || act == CNF_ACT_SOFTPLUS || act == CNF_ACT_SIGMOID ||
           act == CNF_ACT_SWISH || act == CNF_ACT_ELU || act == CNF_ACT_GELU;
}
__device__ __forceinline__ float act_dd_rt(int act, float x, float d) {
    switch (act) {
        case CNF_ACT_IDENTITY: return 0.f;
        case CNF_ACT_TANH: return -2.f * x * d;                        // -2 h act'
        case CNF_ACT_SOFTPLUS: return d * (1.f - d);                   // act' (1 - act')
        case CNF_ACT_SIGMOID: return d * (1.f - 2.f * x);              // act' (1 - 2 h)
        case CNF_ACT_ELU: return x < 0.f ? d : 0.f;                    // exp(a) below 0
        case CNF_ACT_SWISH: {                                          // s (1 - s) (2 + a (1 - 2 s))
            float s, c;
            sigmoid_pair(x, s, c);
            return s * c * fmaf(x, c - s, 2.f);
        }
        case CNF_ACT_GELU: {                                           // 2 s (1 - s) (2 u' + a (2 u'^2 (1 - 2 s) + u''))
            const float t = gelu_tail(x), t2 = t * t;
            float s, c;
            sigmoid_pair(2.f * t * fmaf(kGeluK1, t2, kGeluK0), s, c);
            const float du = fmaf(3.f * kGeluK1, t2, kGeluK0);
            const float inner = fmaf(2.f * du * du, c - s, 6.f * kGeluK1 * t);
            return 2.f * s * c * fmaf(t, inner, 2.f * du);
        }
        default: return __builtin_nanf("");
    }
}

constexpr float kLog2Pi = 1.8378770664093453f;

// "dynamic LDS above 64 KB enabled for this kernel" flag, one bit per device; host threads may race on
// the first launch (the attribute call is idempotent, the flag updates are atomic)
struct DeviceOnce {
    std::atomic<unsigned long long> mask{0};
    bool done(int dev) const { return (mask.load(std::memory_order_acquire) >> (dev & 63)) & 1ull; }
    void set(int dev) { mask.fetch_or(1ull << (dev & 63), std::memory_order_release); }
};

}  // namespace cnf
