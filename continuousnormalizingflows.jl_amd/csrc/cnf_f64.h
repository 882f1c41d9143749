// cnf_f64.h — interface between the double-precision C-ABI layer (cnf_api_f64.hip) and its one kernel (cnf_f64.hip).
#pragma once
#include <string>

#include "cnf_common.h"

namespace cnf {

constexpr int kF64LdsBytes = 160 * 1024;   // LDS of a gfx950 compute unit
constexpr int kF64MaxWaves = 4;            // waves per workgroup at most (one per SIMD); smaller workgroups share a CU

// One Dense layer as the kernel sees it.  Offsets are in doubles into the operand image (f64_pack), `dv_row` in rows of the
// per-wave LDS region.
struct F64Layer {
    int in, out, act;
    int Kp, Mp;        // forward product W h:    K = in  padded to 4,  M = out padded to 16
    int Ko, Mi;        // pullback W^T delta:     K = out padded to 4,  M = in  padded to 16
    int wf, bias, wt;  // image: W as (k, o) -> wf + k Mp + o; bias (Mp); W^T as (o, i) -> wt + o Mi + i; padding is zero
    int dv_row;        // act'_l: Mp rows
};

// The flow and the per-wave LDS layout: every buffer is [row][16 samples] doubles, 128 bytes a row.
struct F64Net {
    int D, S, C, autonomous, L, mode, K, reg_z, reg_j, n_in;
    F64Layer lay[CNF_MAX_LAYERS];
    int x_row;         // layer-one input [z; t; ys], n_in padded to 4 rows
    int p_row[2];      // ping-pong pair, maxM rows each: h_l on the way up, delta_l on the way down
    int u_row;         // ODE state, S rows
    int k_row;         // stage derivatives, ns S rows (ns = 6 when the solver is not known)
    int e_row;         // probes, K D rows (Hutchinson mode)
    int rows;          // rows of one wave's region
    size_t image;      // doubles of the operand image
};

struct F64Args {
    const double* x;     // nvars x B (u0 = [x; 0]) or null
    const double* u0;    // S x B or null
    const double* eps;
    const double* ys;
    long long B;
    int nsteps;          // 0: one dynamics call at t0, du -> u_out
    double t0, dt;
    double* u_out;       // S x B or null
    double* logp;        // B or null
    double* regs;        // 3 B or null
    int nvars, reg_aug;
    TableauD T;          // make_tableau_f64 (cnf_common.h)
};

// rows of one wave's LDS region and the image layout, from the widths alone.  ns = stage derivatives the region keeps: the
// solver's own count for a call (Tsit5 6, RK4 4, one dynamics call 1), 6 for cnf_f64_supported ("under every solver").
// The image layout does not depend on ns.
void f64_layout(const cnf_config& c, F64Net* net, int ns = 6);
// waves per workgroup the LDS budget allows for this flow (0: not even one)
int f64_waves(const F64Net& net);
// W / W^T / bias of every layer, zero-padded, from the Lux-layout vector (both on the device); one kernel per layer on `st`
hipError_t f64_pack(const F64Net& net, const double* lux, const size_t* w_off, const size_t* b_off, double* image, hipStream_t st);
hipError_t f64_solve(const F64Net& net, const double* image, const F64Args& a, hipStream_t st);

}  // namespace cnf
