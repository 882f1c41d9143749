// cnf_f64.hip — the double-precision evaluation path: one kernel, run-time shapes, every product on v_mfma_f64_16x16x4_f64.
//
// One launch is one whole fixed-step solve (nsteps x stages), or one dynamics call (nsteps = 0).  A wave owns a 16-sample tile
// for the whole solve: u0 / x / eps / ys are read once, the outputs written once; the ODE state, the stage derivatives and the
// activations live in the wave's own LDS region (F64Net, cnf_f64.h) - waves never exchange anything, so there is no barrier.
//
// Products.  Samples are the N side (16 columns), a layer's outputs the M side:
//   forward   a_l     = W_l h_{l-1} + b_l          A = W_l   (lane: row o = 16 mt + (lane & 15), k = 4 ks + (lane >> 4))
//   pullback  delta_{l-1} = (W_l^T delta_l) act'_{l-1}   A = W_l^T, from the transposed image
//   B operand = an LDS buffer [k][16]: element (4 ks + (lane >> 4), lane & 15) is at 64 ks + lane - conflict-free
//   C / D     : col = lane & 15, row = (lane >> 4) + 4 reg  (NOT the f32 layout), four doubles per lane
// Widths are not multiples of 16 or 4: the image (f64_pack) pads W, W^T and the biases with zeros, and every LDS row a product
// reads beyond a real width holds 0 (h, delta and act' alike), so padded rows and k-steps contribute exact zeros.
// The trace: Hutchinson probes, or the D unit vectors through the same pullback (CNF_MODE_EXACT).
#include "cnf_f64.h"

namespace cnf {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr double kGeluK0d = 0.7978845608028654;     // sqrt(2 / pi)
constexpr double kGeluK1d = 0.035677408136300125;   // sqrt(2 / pi) * 0.044715
constexpr double kLog2PiD = 1.8378770664093453;

// s = sigmoid(x), c = 1 - s, from e = exp(-|x|) in (0, 1]: no overflow, and the smaller of the two is not formed by cancellation
__device__ __forceinline__ void sigmoid_pair_d(double x, double& s, double& c) {
    const double e = exp(-fabs(x));
    const double r = 1.0 / (1.0 + e);
    const double p = e * r;
    s = x >= 0.0 ? r : p;
    c = x >= 0.0 ? p : r;
}

// h = act(a), d = act'(a): the forms of act_fwd_rt (cnf_common.h) in double with the device libm; ELU takes expm1 where the
// f32 code takes a Taylor branch
__device__ __forceinline__ double act_fwd_d(int act, double a, double& d) {
    switch (act) {
        case CNF_ACT_TANH: {
            const double h = tanh(a);
            d = fma(-h, h, 1.0);
            return h;
        }
        case CNF_ACT_SOFTPLUS: {
            const double e = exp(-fabs(a));
            const double r = 1.0 / (1.0 + e);
            d = a >= 0.0 ? r : e * r;
            return log1p(e) + fmax(a, 0.0);
        }
        case CNF_ACT_SIGMOID: {
            double s, c;
            sigmoid_pair_d(a, s, c);
            d = s * c;
            return s;
        }
        case CNF_ACT_SWISH: {
            double s, c;
            sigmoid_pair_d(a, s, c);
            const double h = a * s;
            d = fma(h, c, s);
            return h;
        }
        case CNF_ACT_ELU: {
            d = a >= 0.0 ? 1.0 : exp(fmin(a, 0.0));
            return a >= 0.0 ? a : expm1(fmin(a, 0.0));
        }
        case CNF_ACT_GELU: {
            const double t = fabs(a) > 1e4 ? copysign(1e4, a) : a, t2 = t * t;   // past |a| ~ 20 sigmoid(2u) is exactly 0 or 1
            double s, c;
            sigmoid_pair_d(2.0 * t * fma(kGeluK1d, t2, kGeluK0d), s, c);
            const double du = fma(3.0 * kGeluK1d, t2, kGeluK0d);
            d = fma(2.0 * t * s * c, du, s);
            return a * s;
        }
        default:
            d = 1.0;
            return a;
    }
}

// LDS traffic of one wave is ordered by the hardware; this keeps the compiler from moving an access across a producer /
// consumer boundary between lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the rows of one sample: a lane holds rows (lane >> 4) + 4 j of column lane & 15
__device__ __forceinline__ double column_sum(double s) {
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    return s;
}

// G output tiles from mt0 on: acc[j](row, col) = sum_k A(16 (mt0 + j) + row, k) in(k, col); G independent accumulator chains.
// The k-steps run in blocks of four, double-buffered: the operands of block kb + 1 (4 G doubles of the image from L2, 4 of the
// LDS buffer) are requested before the 4 G MFMAs of block kb issue, so the L2 latency hides behind the MFMA pipe; the up to
// three k-steps left over run singly.
template <int G>
__device__ __forceinline__ void product_tiles(const double* __restrict__ A, int Mp, int nks, const double* in, int mt0, int lane,
                                              d4 (&acc)[G]) {
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    const double* ap = A + (size_t)(lane >> 4) * Mp + 16 * mt0 + (lane & 15);
    const double* bp = in + lane;
    const size_t kstep = 4 * (size_t)Mp;
    const int nb = nks >> 2;
    double a0[4][G], b0[4];
    if (nb > 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            b0[u] = bp[64 * u];
#pragma unroll
            for (int j = 0; j < G; ++j) a0[u][j] = ap[u * kstep + 16 * j];
        }
    }
    for (int kb = 0; kb < nb; ++kb) {
        const int nx = kb + 1 < nb ? kb + 1 : kb;   // the last block asks for itself again: in bounds, unused
        const double* an = ap + 4 * nx * kstep;
        const double* bn = bp + 256 * nx;
        double a1[4][G], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            b1[u] = bn[64 * u];
#pragma unroll
            for (int j = 0; j < G; ++j) a1[u][j] = an[u * kstep + 16 * j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < G; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u][j], b0[u], acc[j], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            b0[u] = b1[u];
#pragma unroll
            for (int j = 0; j < G; ++j) a0[u][j] = a1[u][j];
        }
    }
    for (int ks = 4 * nb; ks < nks; ++ks) {
        const double b = bp[64 * ks];
#pragma unroll
        for (int j = 0; j < G; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[ks * kstep + 16 * j], b, acc[j], 0, 0, 0);
    }
}

template <int G, class Epi>
__device__ __forceinline__ void product_group(const double* __restrict__ A, int Mp, int nks, const double* in, int mt0, int lane, Epi& epi) {
    d4 acc[G];
    product_tiles<G>(A, Mp, nks, in, mt0, lane, acc);
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) epi(16 * (mt0 + j) + (lane >> 4) + 4 * r, acc[j][r]);
}

// out(row, col) = epi(row, sum_k A(row, k) in(k, col)) for the nmt row tiles, in groups of up to four tiles that share the
// LDS operand (5 tiles run as 3 + 2, not 4 + 1: a lone tile is one dependent chain); epi also stores
template <class Epi>
__device__ __forceinline__ void product(const double* __restrict__ A, int Mp, int nks, const double* in, int nmt, int lane, Epi epi) {
    for (int mt0 = 0; mt0 < nmt;) {
        const int rem = nmt - mt0;
        const int g = rem <= 4 ? rem : (rem >= 8 ? 4 : (rem + 1) >> 1);
        if (g == 4) product_group<4>(A, Mp, nks, in, mt0, lane, epi);
        else if (g == 3) product_group<3>(A, Mp, nks, in, mt0, lane, epi);
        else if (g == 2) product_group<2>(A, Mp, nks, in, mt0, lane, epi);
        else product_group<1>(A, Mp, nks, in, mt0, lane, epi);
        mt0 += g;
    }
}

// One dynamics evaluation of the wave's tile: the layer-one input X holds [z; t; ys]; kout (S rows) receives [zdot; ldot; Edot; ndot]
__device__ __forceinline__ void dynamics(const F64Net& net, const double* __restrict__ img, double* R, double* kout, int lane) {
    const int n = lane & 15, q = lane >> 4;
    const int D = net.D, L = net.L;
    // forward chain: h_l into the ping-pong pair, act'_l kept for the pullback
    const double* in = R + 16 * net.x_row;
    for (int l = 0; l < L; ++l) {
        const F64Layer& ly = net.lay[l];
        double* out = R + 16 * net.p_row[l & 1];
        double* dv = R + 16 * ly.dv_row;
        const double* bias = img + ly.bias;
        const int act = ly.act, nout = ly.out;
        product(img + ly.wf, ly.Mp, ly.Kp >> 2, in, ly.Mp >> 4, lane, [&](int row, double v) { out[16 * row + n] = v + bias[row]; });
        // the activation as one loop over the lane's own results (the libm code once, not once per accumulator register);
        // padded rows keep h = 0 and get act' = 0
        for (int r = q; r < ly.Mp; r += 4) {
            double d = 0.0;
            if (r < nout) out[16 * r + n] = act_fwd_d(act, out[16 * r + n], d);
            dv[16 * r + n] = d;
        }
        wave_sync();
        in = out;
    }
    // zdot and |zdot|
    double e2 = 0.0;
    for (int r = q; r < D; r += 4) {
        const double z = in[16 * r + n];
        kout[16 * r + n] = z;
        e2 = fma(z, z, e2);
    }
    e2 = column_sum(e2);
    const double Edot = (net.reg_z && net.mode != CNF_MODE_EXACT) ? sqrt(e2) : 0.0;
    wave_sync();   // the pair is free again
    // pullback, probe by probe: delta_L = probe . act'_L, down to the cotangent of z
    const bool exact = net.mode == CNF_MODE_EXACT;
    const int nprobe = exact ? D : net.K;
    const double* eps = R + 16 * net.e_row;
    const double* dvL = R + 16 * net.lay[L - 1].dv_row;
    const int Ko_last = net.lay[L - 1].Ko;
    double ldot = 0.0, ndot = 0.0;
    for (int p = 0; p < nprobe; ++p) {
        double* cur = R + 16 * net.p_row[L & 1];
        for (int r = q; r < Ko_last; r += 4) {
            const double s = r < D ? (exact ? (r == p ? 1.0 : 0.0) : eps[16 * (p * D + r) + n]) : 0.0;
            cur[16 * r + n] = s * dvL[16 * r + n];
        }
        wave_sync();
        for (int l = L - 1; l >= 0; --l) {
            const F64Layer& ly = net.lay[l];
            double* out = R + 16 * net.p_row[l & 1];
            const int nmt = l > 0 ? ly.Mi >> 4 : (D + 15) >> 4;   // of layer one's input only the z rows are wanted
            if (l > 0) {
                const double* dv = R + 16 * net.lay[l - 1].dv_row;
                product(img + ly.wt, ly.Mi, ly.Ko >> 2, cur, nmt, lane,
                        [&](int row, double v) { out[16 * row + n] = v * dv[16 * row + n]; });
            } else {
                product(img + ly.wt, ly.Mi, ly.Ko >> 2, cur, nmt, lane, [&](int row, double v) { out[16 * row + n] = v; });
            }
            wave_sync();
            cur = out;
        }
        // cur rows 0 .. D-1: g = probe^T J
        if (exact) {
            if (q == 0) ldot -= cur[16 * p + n];
        } else {
            double ge = 0.0, g2 = 0.0;
            for (int r = q; r < D; r += 4) {
                const double g = cur[16 * r + n];
                ge = fma(g, eps[16 * (p * D + r) + n], ge);
                g2 = fma(g, g, g2);
            }
            ldot -= column_sum(ge);
            if (net.reg_j) ndot += sqrt(column_sum(g2));
        }
        wave_sync();
    }
    if (!exact) {
        ldot /= (double)net.K;
        ndot /= (double)net.K;
    }
    if (q == 0) {
        kout[16 * D + n] = ldot;
        kout[16 * (D + 1) + n] = Edot;
        kout[16 * (D + 2) + n] = ndot;
    }
    wave_sync();
}

__global__ __launch_bounds__(64 * kF64MaxWaves) void f64_solve_kernel(const F64Net net, const F64Args a, const double* __restrict__ img) {
    extern __shared__ double f64_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long long tile = (long long)blockIdx.x * nw + wave;
    if (tile * 16 >= a.B) return;
    double* R = f64_lds + (size_t)wave * net.rows * 16;
    const int n = lane & 15, q = lane >> 4;
    const int D = net.D, S = net.S;
    const long long col = tile * 16 + n;
    const bool live = col < a.B;   // a ragged tile's spare columns compute on zeros and store nothing
    double* X = R + 16 * net.x_row;
    double* U = R + 16 * net.u_row;
    double* Kb = R + 16 * net.k_row;
    // inputs, once per solve
    for (int r = q; r < S; r += 4) {
        double v = 0.0;
        if (live) {
            if (a.u0) v = a.u0[col * S + r];
            else if (r < a.nvars) v = a.x[col * a.nvars + r];
        }
        U[16 * r + n] = v;
    }
    const int xr = (net.n_in + 3) & ~3;
    const int yrow = D + (net.autonomous ? 0 : 1);
    for (int r = q; r < xr; r += 4) {
        double v = 0.0;
        if (live && r >= yrow && r < net.n_in) v = a.ys[col * net.C + (r - yrow)];
        X[16 * r + n] = v;
    }
    if (net.mode != CNF_MODE_EXACT) {
        double* E = R + 16 * net.e_row;
        const int KD = net.K * D;
        for (int r = q; r < KD; r += 4) E[16 * r + n] = live ? a.eps[col * KD + r] : 0.0;
    }
    wave_sync();
    if (a.nsteps == 0) {
        for (int r = q; r < D; r += 4) X[16 * r + n] = U[16 * r + n];
        if (!net.autonomous && q == 0) X[16 * D + n] = a.t0;
        wave_sync();
        dynamics(net, img, R, Kb, lane);
        if (live && a.u_out)
            for (int r = q; r < S; r += 4) a.u_out[col * S + r] = Kb[16 * r + n];
        return;
    }
    const int ns = a.T.ns;
    const double dt = a.dt;
    for (int step = 0; step < a.nsteps; ++step) {
        const double tn = a.t0 + (double)step * dt;
        for (int i = 0; i < ns; ++i) {
            // stage state (z rows only: the dynamics do not read the other three) straight into the layer-one input
            for (int r = q; r < D; r += 4) {
                double v = U[16 * r + n];
                for (int j = 0; j < i; ++j) v = fma(dt * a.T.a[i][j], Kb[16 * (j * S + r) + n], v);
                X[16 * r + n] = v;
            }
            if (!net.autonomous && q == 0) X[16 * D + n] = tn + a.T.c[i] * dt;
            wave_sync();
            dynamics(net, img, R, Kb + 16 * i * S, lane);
        }
        for (int r = q; r < S; r += 4) {
            double v = U[16 * r + n];
            for (int j = 0; j < ns; ++j) v = fma(dt * a.T.b[j], Kb[16 * (j * S + r) + n], v);
            U[16 * r + n] = v;
        }
        wave_sync();
    }
    // outputs, once per solve
    if (a.u_out && live)
        for (int r = q; r < S; r += 4) a.u_out[col * S + r] = U[16 * r + n];
    if (a.logp) {
        double z2 = 0.0, a2 = 0.0;
        for (int r = q; r < D; r += 4) {
            const double z = U[16 * r + n];
            z2 = fma(z, z, z2);
            if (r >= a.nvars) a2 = fma(z, z, a2);
        }
        z2 = column_sum(z2);
        a2 = column_sum(a2);
        if (live && q == 0) {
            a.logp[col] = -0.5 * (double)D * kLog2PiD - 0.5 * z2 - U[16 * D + n];
            if (a.regs) {
                a.regs[col] = U[16 * (D + 1) + n];
                a.regs[a.B + col] = U[16 * (D + 2) + n];
                a.regs[2 * a.B + col] = a.reg_aug ? sqrt(a2) : 0.0;
            }
        }
    }
}

// image of one layer: W as (k, o), the bias, W^T as (o, i); everything beyond a real width is zero
__global__ void f64_pack_kernel(F64Layer ly, const double* __restrict__ lux, size_t w_off, size_t b_off, double* __restrict__ image) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int nf = ly.Mp * ly.Kp, nt = ly.Mi * ly.Ko;
    if (j < nf) {
        const int k = j / ly.Mp, o = j - k * ly.Mp;
        image[ly.wf + j] = (k < ly.in && o < ly.out) ? lux[w_off + (size_t)o + (size_t)ly.out * k] : 0.0;
    } else if (j < nf + ly.Mp) {
        const int o = j - nf;
        image[ly.bias + o] = o < ly.out ? lux[b_off + o] : 0.0;
    } else if (j < nf + ly.Mp + nt) {
        const int e = j - nf - ly.Mp;
        const int o = e / ly.Mi, i = e - o * ly.Mi;
        image[ly.wt + e] = (o < ly.out && i < ly.in) ? lux[w_off + (size_t)o + (size_t)ly.out * i] : 0.0;
    }
}

}  // namespace

void f64_layout(const cnf_config& c, F64Net* net, int ns) {
    F64Net& n = *net;
    n = F64Net{};
    n.D = c.nvars + c.naug;
    n.S = n.D + 3;
    n.C = c.ncond;
    n.autonomous = c.autonomous;
    n.L = c.n_layers;
    n.mode = c.mode;
    n.K = c.nprobes;
    n.reg_z = c.reg_z;
    n.reg_j = c.reg_j;
    n.n_in = c.widths[0];
    size_t off = 0;
    int row = 0, maxM = 16;
    n.x_row = row;
    row += (n.n_in + 3) & ~3;
    for (int l = 0; l < c.n_layers; ++l) {
        F64Layer& ly = n.lay[l];
        ly.in = c.widths[l];
        ly.out = c.widths[l + 1];
        ly.act = c.acts[l];
        ly.Kp = (ly.in + 3) & ~3;
        ly.Mp = (ly.out + 15) & ~15;
        ly.Ko = (ly.out + 3) & ~3;
        ly.Mi = (ly.in + 15) & ~15;
        ly.wf = (int)off;   off += (size_t)ly.Mp * ly.Kp;
        ly.bias = (int)off; off += (size_t)ly.Mp;
        ly.wt = (int)off;   off += (size_t)ly.Mi * ly.Ko;
        ly.dv_row = row;
        row += ly.Mp;
        if (ly.Mp > maxM) maxM = ly.Mp;
        if (ly.Mi > maxM) maxM = ly.Mi;
    }
    n.p_row[0] = row; row += maxM;
    n.p_row[1] = row; row += maxM;
    n.u_row = row;    row += n.S;
    n.k_row = row;    row += ns * n.S;
    n.e_row = row;    row += c.mode == CNF_MODE_EXACT ? 0 : n.K * n.D;
    n.rows = row;
    n.image = off;
}

int f64_waves(const F64Net& net) {
    const long long per_wave = 128LL * net.rows;   // bytes: 16 doubles a row
    const long long fit = kF64LdsBytes / per_wave;
    return (int)(fit < kF64MaxWaves ? fit : kF64MaxWaves);
}

hipError_t f64_pack(const F64Net& net, const double* lux, const size_t* w_off, const size_t* b_off, double* image, hipStream_t st) {
    for (int l = 0; l < net.L; ++l) {
        const F64Layer& ly = net.lay[l];
        const int total = ly.Mp * ly.Kp + ly.Mp + ly.Mi * ly.Ko;
        hipLaunchKernelGGL(f64_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, ly, lux, w_off[l], b_off[l], image);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t f64_solve(const F64Net& net, const double* image, const F64Args& a, hipStream_t st) {
    const int nw = f64_waves(net);
    if (nw < 1) return hipErrorNotSupported;
    static DeviceOnce once;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!once.done(dev)) {
        e = hipFuncSetAttribute((const void*)f64_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kF64LdsBytes);
        if (e != hipSuccess) return e;
        once.set(dev);
    }
    const long long ntiles = (a.B + 15) / 16;
    const long long nblocks = (ntiles + nw - 1) / nw;
    if (nblocks < 1 || nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = (size_t)nw * net.rows * 128;
    hipLaunchKernelGGL(f64_solve_kernel, dim3((unsigned)nblocks), dim3(64 * nw), lds, st, net, a, image);
    return hipGetLastError();
}

}  // namespace cnf
