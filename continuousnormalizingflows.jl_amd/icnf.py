"""Host-side mirror of the reference's AbstractICNF interface for the batched (MatrixMode)
fixed-step path, sitting directly on the C ABI of libcnf_hip.so.

The reference is Julia (no Julia toolchain in this image), so this module plays the role the
`HIPMatrixMode` glue of INTEGRATION.md plays there: same names, argument order, array shapes
((rows, B), one column per sample) and error behaviour as the reference's `ICNF`, `inference`,
`generate`, `loss`, `TrainMode`/`TestMode` and ComputeMode types, so the parity tests read like
the reference's smoke tests (test/ci_tests/smoke_tests.jl).  torch is used only for device
memory, streams, RNG and torch.distributed.

Reference map (relative to the reference repo):
  ICNF(; ...)                      src/core/icnf.jl:53-141
  TrainMode / TestMode             src/core/types.jl:1-7
  *MatrixMode compute modes        src/core/types.jl:9-35
  inference / generate             src/core/base_icnf.jl:406-465
  loss                             src/core/icnf.jl:628-649
  (icnf)(xs, ps, st)               src/core/base_icnf.jl:509-523
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import ptr as _ptr, stream_ptr as _stream_ptr
from .solvers import _adaptive_integrate, _solve_errors, _vcabm_integrate  # noqa: F401

__all__ = [
    "ICNF", "TrainMode", "TestMode", "Dense", "Chain", "PlanarLayer", "tanh", "softplus", "identity",
    "sigmoid", "swish", "elu", "gelu",
    "HIPVecJacMatrixMode", "HIPJacVecMatrixMode", "LuxVecJacMatrixMode", "LuxJacVecMatrixMode",
    "DIVecJacMatrixMode", "DIJacVecMatrixMode", "Tsit5", "RK4", "VCABM", "setup", "inference", "generate",
    "loss", "augmented_f", "loss_and_gradient", "integrate_vjp", "vjp_path",
]


# ---------------------------------------------------------------------------------------
# modes (src/core/types.jl)
# ---------------------------------------------------------------------------------------
class Mode:
    pass


class TestMode(Mode):
    __test__ = False  # not a pytest class

    def __repr__(self):
        return "TestMode()"


class TrainMode(Mode):
    """TrainMode{REG}; TrainMode() == TrainMode{true}() (src/core/types.jl:5-7)."""

    def __init__(self, reg: bool = True):
        self.reg = bool(reg)

    def __repr__(self):
        return f"TrainMode{{{str(self.reg).lower()}}}()"


class ComputeMode:
    jacvec = False


class MatrixMode(ComputeMode):
    """Whole batch in one solve.  `kernel_path` is PATH_AUTO / PATH_SIMT / PATH_MFMA."""

    def __init__(self, adback=None, kernel_path: int = _lib.PATH_AUTO, arith: int = _lib.ARITH_F32):
        self.adback = adback  # accepted for signature parity; AD is hand-written in the kernels
        self.kernel_path = kernel_path
        self.arith = arith    # ARITH_F32 (exact, default) or ARITH_BF16X6 (split-bf16 MFMA)


class HIPVecJacMatrixMode(MatrixMode):
    jacvec = False


class HIPJacVecMatrixMode(MatrixMode):
    jacvec = True


# The reference's MatrixMode names select the same estimators; they resolve to the HIP kernels.
LuxVecJacMatrixMode = DIVecJacMatrixMode = HIPVecJacMatrixMode
LuxJacVecMatrixMode = DIJacVecMatrixMode = HIPJacVecMatrixMode


# ---------------------------------------------------------------------------------------
# network description (Lux.Chain of Lux.Dense, src/core/icnf.jl:67-71)
# ---------------------------------------------------------------------------------------
def identity(x):
    return x


def tanh(x):
    return torch.tanh(x)


def softplus(x):
    return torch.nn.functional.softplus(x)


def sigmoid(x):
    return torch.sigmoid(x)


def swish(x):
    return x * torch.sigmoid(x)


def elu(x):
    return torch.nn.functional.elu(x)


def gelu(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


# the module functions, one per activation id (include/cnf.h CNF_ACT_*); each id's canonical name is its function's name
_ACT_FUNCS = {identity: _lib.ACT_IDENTITY, tanh: _lib.ACT_TANH, softplus: _lib.ACT_SOFTPLUS, sigmoid: _lib.ACT_SIGMOID,
              swish: _lib.ACT_SWISH, elu: _lib.ACT_ELU, gelu: _lib.ACT_GELU}
_ACT_NAMES = {i: f.__name__ for f, i in _ACT_FUNCS.items()}   # id -> name (the machine file stores names)
_ACT_IDS = {**_ACT_FUNCS, **{n: i for i, n in _ACT_NAMES.items()}, None: _lib.ACT_IDENTITY,
            torch.sigmoid: _lib.ACT_SIGMOID, torch.nn.functional.silu: _lib.ACT_SWISH, "silu": _lib.ACT_SWISH}


@dataclass
class Dense:
    """Dense(in => out, activation)."""
    n_in: int
    n_out: int
    activation: Union[Callable, str, None] = identity

    @property
    def act_id(self) -> int:
        try:
            return _ACT_IDS[self.activation]
        except KeyError:
            raise TypeError(f"MethodError: no HIP kernel for activation {self.activation!r} "
                            "(supported: identity, tanh, softplus, sigmoid, swish, elu, gelu)") from None


@dataclass
class PlanarLayer:
    """PlanarLayer(in => out, activation): z -> u * activation(w' z + b)  (src/layers/planar_layer.jl:6-77).
    It is the Dense chain Dense(in => 1, activation) -> Dense(1 => out) with the second bias pinned to zero,
    so it runs on the same kernels; only the parameter order differs: ps = (u (out), w (in), b (1))
    (src/layers/planar_layer.jl:36-50).  Use it as `nn=Chain(PlanarLayer(...))` like the reference's tests
    (test/ci_tests/smoke_tests.jl:32-46)."""
    n_in: int
    n_out: int
    activation: Union[Callable, str, None] = identity
    use_bias: bool = True


class Chain:
    def __init__(self, *layers):
        if not layers:
            raise ValueError("Chain needs at least one Dense layer")
        self.planar = None
        if len(layers) == 1 and isinstance(layers[0], PlanarLayer):
            pl = layers[0]
            self.planar = pl
            layers = (Dense(pl.n_in, 1, pl.activation), Dense(1, pl.n_out, identity))
        elif any(isinstance(l, PlanarLayer) for l in layers):
            raise TypeError("MethodError: PlanarLayer is supported as the only layer of the Chain")
        for a, b in zip(layers[:-1], layers[1:]):
            if a.n_out != b.n_in:
                raise ValueError(f"DimensionMismatch: Dense({a.n_in}=>{a.n_out}) followed by "
                                 f"Dense({b.n_in}=>{b.n_out})")
        self.layers = tuple(layers)

    @property
    def widths(self):
        return [self.layers[0].n_in] + [l.n_out for l in self.layers]

    def param_offsets(self):
        """ComponentArray layout: layer_k.weight (out x in, column-major), layer_k.bias.
        For a PlanarLayer: (u, w, b); the ABI view appends the pinned zero bias (and a zero b when
        use_bias = false) behind the user's vector — see abi_params."""
        if self.planar is not None:
            pl = self.planar
            n_user = pl.n_out + pl.n_in + (1 if pl.use_bias else 0)
            b0 = pl.n_out + pl.n_in if pl.use_bias else n_user + pl.n_out   # b, or an appended zero
            return [pl.n_out, 0], [b0, n_user], n_user
        w_off, b_off, o = [], [], 0
        for l in self.layers:
            w_off.append(o)
            o += l.n_in * l.n_out
            b_off.append(o)
            o += l.n_out
        return w_off, b_off, o

    def abi_params(self, ps: torch.Tensor) -> torch.Tensor:
        """The vector handed to cnf_set_params: ps itself for Dense chains; for a PlanarLayer ps followed
        by the zeros that stand for the absent biases."""
        if self.planar is None:
            return ps
        pad = self.planar.n_out + (0 if self.planar.use_bias else 1)
        return torch.cat([ps, torch.zeros(pad, dtype=ps.dtype, device=ps.device)])


# ---------------------------------------------------------------------------------------
# solver selection (sol_kwargs.alg)
# ---------------------------------------------------------------------------------------
class Tsit5:
    alg_id = _lib.ALG_TSIT5


class RK4:
    alg_id = _lib.ALG_RK4


class VCABM:
    """The reference's default algorithm (src/core/icnf.jl:84-89): adaptive order (1..12), adaptive step Adams
    predictor-corrector (OrdinaryDiffEqAdamsBashforthMoulton.VCABM).  Always adaptive here."""
    alg_id = _lib.ALG_VCABM


# ---------------------------------------------------------------------------------------
# ICNF
# ---------------------------------------------------------------------------------------
class _DTypeMismatch(TypeError, ValueError):
    """A tensor whose precision is not the flow's data_type.  A TypeError; also a ValueError, which is what a non-Float32 `ps`
    raised before Float64 flows existed."""


class _Handle:
    """Owns one cnf_handle (one trace mode / regulariser combination)."""

    def __init__(self, cfg: _lib.CnfConfig):
        self.lib = _lib.load()
        self.ptr = C.c_void_p()
        _lib.check(self.lib.cnf_create(C.byref(self.ptr), C.byref(cfg)))
        self.params_key = None
        self.params_ref = None

    def __del__(self):
        try:
            if self.ptr:
                self.lib.cnf_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


class ICNF:
    """Keyword constructor mirroring `ICNF(; ...)` (src/core/icnf.jl:53-103).

    Differences forced by the fixed-step HIP path (all raise instead of silently falling back):
      * `sol_kwargs.alg` is VCABM() (the reference's default when none is given), Tsit5() or RK4().  Tsit5 / RK4 with
        adaptive=False (and `dt` or `nsteps`): the whole solve is one fused launch.  VCABM() and Tsit5() with
        adaptive=True (OrdinaryDiffEq's default; reltol/abstol default 1e-4 as in the reference) step under the
        solver's controller on the host with one device attempt per step (`_vcabm_integrate`, `_adaptive_integrate`).
      * `nn` must be a Chain of Dense layers with identity/tanh/softplus/sigmoid/swish/elu/gelu activations
        (elu with alpha = 1, gelu in its tanh form).  Nets with sigmoid, swish, elu or gelu hidden layers run
        layer-wise (or thread-per-sample for layers wider than 512): the fused kernels are built for tanh and softplus.
      * data_type is Float32 (every entry point) or Float64.  A Float64 flow evaluates - augmented_f, inference, generate, loss,
        logpdf / rand - with fixed-step Tsit5() / RK4() (adaptive=False and nsteps or dt) on the double-precision kernel
        (csrc/cnf_f64.hip), takes and returns float64 tensors and casts nothing silently; adaptive stepping, VCABM, gradients and
        fit are Float32 only and raise NotImplementedError on a Float64 flow.  Its `nsteps` form keeps t0 and t1 in double;
        its `dt` form steps on the plan of the Float32 entries (fixed_dt_grid), which is made from the FLOAT32 values of t0, t1
        and dt: dt=0.3 steps by 0.30000001192..., and an end point a Float32 cannot hold moves by up to 6e-8 relative.  Give
        `nsteps` where the span must be exact in double.
    """

    def __init__(self, *, data_type=torch.float32, compute_mode: Optional[ComputeMode] = None,
                 inplace: bool = False, autonomous: bool = False, device=None, rng=None,
                 tspan: Tuple[float, float] = (0.0, 1.0), nvariables: int = 1,
                 naugments: Optional[int] = None, nconditions: int = 0, n_in: Optional[int] = None,
                 n_out: Optional[int] = None, n_hidden: Optional[int] = None,
                 nn: Optional[Chain] = None, steer_rate: float = 0.1, lambda1: float = 0.01,
                 lambda2: float = 0.01, lambda3: float = 0.01, nprobes: int = 1,
                 basedist=None, epsdist=None, sol_kwargs: Optional[dict] = None, **aliases):
        # accept the reference's unicode keyword names too
        lambda1 = aliases.pop("λ₁", lambda1)
        lambda2 = aliases.pop("λ₂", lambda2)
        lambda3 = aliases.pop("λ₃", lambda3)
        if aliases:
            raise TypeError(f"MethodError: unknown keyword(s) {sorted(aliases)}")
        if data_type is not torch.float32 and data_type is not torch.float64:
            raise TypeError("MethodError: the HIP path computes in Float32 or Float64")
        self.data_type = data_type
        self.f64 = data_type is torch.float64
        self.compute_mode = compute_mode if compute_mode is not None else HIPVecJacMatrixMode()
        if not isinstance(self.compute_mode, MatrixMode):
            raise TypeError("MethodError: only MatrixMode compute modes are implemented "
                            "(VectorMode solves one sample at a time and is out of scope)")
        self.inplace = bool(inplace)
        self.autonomous = bool(autonomous)
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise TypeError("MethodError: HIPMatrixMode needs a cuda (ROCm) device; "
                            "there is no CPU fallback")
        self.tspan = (float(tspan[0]), float(tspan[1]))
        self.nvariables = int(nvariables)
        self.naugments = int(nvariables + 1 if naugments is None else naugments)  # icnf.jl:62
        self.nconditions = int(nconditions)
        D = self.nvariables + self.naugments
        n_in = D + (0 if autonomous else 1) + self.nconditions if n_in is None else n_in
        n_out = D if n_out is None else n_out
        n_hidden = 4 * n_in if n_hidden is None else n_hidden
        if nn is None:  # icnf.jl:67-71
            nn = Chain(Dense(n_in, n_hidden, softplus), Dense(n_hidden, n_hidden, softplus),
                       Dense(n_hidden, n_out))
        if not isinstance(nn, Chain):
            raise TypeError("MethodError: nn must be a Chain of Dense layers")
        self.nn = nn
        self.steer_rate = float(steer_rate)
        self.lambda1, self.lambda2, self.lambda3 = float(lambda1), float(lambda2), float(lambda3)
        self.nprobes = int(nprobes)
        # basedist / epsdist (src/core/icnf.jl:76-83): None = MvNormal(0, I), the case the kernels fuse
        # (log N(z) in the epilogue, z ~ N(0, I) in generate, Gaussian probes).  basedist may be any object with
        # `log_prob(z)` and `sample((n,))` on (n, D) tensors (torch.distributions style): logpdf(basedist, z) is
        # then evaluated on the host from the final state (base_icnf.jl:168), and the parameter gradient,
        # whose terminal costate assumes the Gaussian, is refused.  epsdist: None, "rademacher", or a callable
        # (generator, (B, K*D), device) -> tensor.
        self.basedist = basedist
        self.epsdist = epsdist
        if basedist is not None and not (hasattr(basedist, "log_prob") and hasattr(basedist, "sample")):
            raise TypeError("MethodError: basedist needs log_prob(z) and sample((n,))")
        if epsdist is not None and epsdist != "rademacher" and not callable(epsdist):
            raise TypeError("MethodError: epsdist is None, 'rademacher' or a callable")
        # icnf.rng draws the Hutchinson probes (base_icnf.jl:258-259).  When the columns are sharded over ranks each
        # rank must draw DIFFERENT probes for its columns, so the default generator is seeded with the rank; the STEER
        # end time (one draw per call for the whole batch, base_icnf.jl:23-43) comes from a second generator that is
        # seeded identically on every rank, so all shards integrate the same span (drawing it from the
        # per-rank stream desynchronises the ranks).  `sharded=False` makes every call of this ICNF rank-local (no
        # collectives even though a process group exists); None = follow torch.distributed / the installed Comm.
        self.rng = rng
        self.sharded: Optional[bool] = None
        rank = 0
        try:
            import torch.distributed as _d
            if _d.is_available() and _d.is_initialized():
                rank = _d.get_rank()
        except Exception:
            rank = 0
        if self.rng is None and torch.cuda.is_available():
            self.rng = torch.Generator(device=self.device)
            self.rng.manual_seed(rank)
        self.steer_rng = torch.Generator(device="cpu")
        self.steer_rng.manual_seed(0)
        self.sol_kwargs = dict(sol_kwargs or {})
        self._handles: Dict[tuple, _Handle] = {}
        w = nn.widths
        if w[0] != D + (0 if autonomous else 1) + self.nconditions or w[-1] != D:
            raise ValueError(
                f"DimensionMismatch: nn maps {w[0]} => {w[-1]} but the flow needs "
                f"{D + (0 if autonomous else 1) + self.nconditions} => {D}")
        if len(nn.layers) > _lib.MAX_LAYERS:
            raise ValueError(f"at most {_lib.MAX_LAYERS} Dense layers are supported")

    # -- type-parameter style flags (src/core/icnf.jl:105-125) --
    @property
    def D(self) -> int:
        return self.nvariables + self.naugments

    @property
    def S(self) -> int:
        return self.D + 3  # n_augments == 2 always (icnf.jl:143-145) plus dlogp

    @property
    def conditioned(self) -> bool:
        return self.nconditions != 0

    @property
    def augmented(self) -> bool:
        return self.naugments != 0

    def _solver(self):
        kw = self.sol_kwargs
        alg = kw.get("alg")
        if alg is None:   # the reference's default: sol_kwargs = (alg = VCABM(), reltol = abstol = 1e-4, ...) (src/core/icnf.jl:84-89)
            alg = VCABM()
            kw["alg"] = alg
        if not hasattr(alg, "alg_id"):
            raise NotImplementedError("sol_kwargs.alg must be VCABM(), Tsit5() or RK4() (other OrdinaryDiffEq algorithms "
                                      "are not implemented)")
        if kw.get("adaptive", True) and alg.alg_id == _lib.ALG_RK4:
            raise NotImplementedError("adaptive stepping is implemented for VCABM() and Tsit5(); use adaptive=False with RK4()")
        if not kw.get("adaptive", True) and alg.alg_id == _lib.ALG_VCABM:
            raise NotImplementedError("VCABM() is implemented as an adaptive solver only; use Tsit5() or RK4() with adaptive=False")
        return alg.alg_id

    @property
    def adaptive(self) -> bool:
        """OrdinaryDiffEq's default: an algorithm with an embedded pair steps adaptively unless adaptive=false."""
        self._solver()
        return bool(self.sol_kwargs.get("adaptive", True))

    def _nsteps(self, t0: float, t1: float) -> int:
        """`nsteps` equal steps (an extension of this host: sol_kwargs.nsteps); with `dt` the solve goes through the
        `*_fixed_dt` entries instead (see _fixed_dt)."""
        kw = self.sol_kwargs
        if "nsteps" in kw:
            return int(kw["nsteps"])
        if "dt" not in kw:
            raise NotImplementedError("sol_kwargs needs dt (or nsteps) with adaptive=False")
        n = abs(t1 - t0) / float(kw["dt"])
        return max(1, int(round(n)))

    def _fixed_dt(self) -> Optional[float]:
        """sol_kwargs = (alg, adaptive = false, dt): OrdinaryDiffEq's fixed-dt stepping — steps of dt and a shorter last
        step onto t1 (what a STEER-drawn t1 meets, base_icnf.jl:23-43) — served by cnf_inference_fixed_dt /
        cnf_integrate_fixed_dt.  None when the user gave `nsteps` (equal steps) instead."""
        kw = self.sol_kwargs
        if "nsteps" in kw or "dt" not in kw:
            return None
        return C.c_float(abs(float(kw["dt"]))).value       # the Float32 the ABI receives: one plan on both sides

    @staticmethod
    def fixed_dt_grid(t0: float, t1: float, dt: float):
        """The times of those steps, [t0, ..., t1]: the plan of cnf_integrate_fixed_dt (fixed_dt_plan, csrc/cnf_api.hip),
        computed like there in double from the Float32 values of t0, t1 and dt that cross the ABI."""
        t0, t1, dt = (C.c_float(float(v)).value for v in (t0, t1, dt))
        span, adt = abs(t1 - t0), abs(dt)
        tdir = 1.0 if t1 >= t0 else -1.0
        n = int(math.floor(span / adt + 1e-9))
        tol = 100.0 * 1.1920928955078125e-7 * max(abs(t0), abs(t1))
        if span - n * adt > tol and adt - (span - n * adt) <= tol:
            n += 1                       # a Float32 dt a hair above span / n: the last step is snapped onto t1, no tail
        if span - n * adt <= tol:
            return [t0] if n == 0 else [t0 + (t1 - t0) * i / n for i in range(n)] + [t1]
        return [t0 + tdir * adt * i for i in range(n + 1)] + [t1]

    def _steer_tspan(self, mode: Mode) -> Tuple[float, float]:
        """steer_tspan (src/core/base_icnf.jl:23-43)."""
        t0, t1 = self.tspan
        if self.steer_rate != 0.0 and isinstance(mode, TrainMode) and mode.reg:
            r = (torch.rand((), generator=self.steer_rng, dtype=torch.float32).item() * 2.0 - 1.0) * self.steer_rate
            t1 = t1 + abs(t1 - t0) * r
        return t0, t1

    def _group(self, group):
        """The `group` argument the reductions and adaptive loops receive: False (rank-local) when this ICNF opted out."""
        return False if self.sharded is False else group

    def invalidate_params(self) -> None:
        """Force the next call to repack `ps` (cnf_set_params).  The binding is skipped only for the SAME tensor object
        at an unchanged `ps._version`; writes that bypass autograd's version counter (through `ps.data`, a raw pointer,
        another library's kernel) must be followed by this call."""
        for h in self._handles.values():
            h.params_key = None
            h.params_ref = None

    def _handle(self, mode: Mode) -> _Handle:
        train = isinstance(mode, TrainMode)
        if not train and not isinstance(mode, TestMode):
            raise TypeError(f"MethodError: no method for mode {mode!r}")
        reg = train and mode.reg
        if not train:
            tmode = _lib.MODE_EXACT
        else:
            tmode = _lib.MODE_HUTCH_JVP if self.compute_mode.jacvec else _lib.MODE_HUTCH_VJP
        reg_z = int(reg and self.lambda1 != 0.0)               # NORM_Z   (icnf.jl:113)
        reg_j = int(reg and self.lambda2 != 0.0)               # NORM_J   (icnf.jl:114)
        reg_aug = int(reg and self.lambda3 != 0.0 and self.augmented)  # NORM_Z_AUG
        nprobes = self.nprobes if train else 1
        arith = getattr(self.compute_mode, "arith", _lib.ARITH_F32)
        # everything the library bakes into the handle (the reference's ICNF is immutable; here fields may be reassigned)
        key = (tmode, reg_z, reg_j, reg_aug, nprobes, self.compute_mode.kernel_path, arith)
        h = self._handles.get(key)
        if h is None:
            cfg = _lib.CnfConfig()
            cfg.nvars, cfg.naug, cfg.ncond = self.nvariables, self.naugments, self.nconditions
            cfg.autonomous = int(self.autonomous)
            cfg.n_layers = len(self.nn.layers)
            for i, wd in enumerate(self.nn.widths):
                cfg.widths[i] = wd
            for i, l in enumerate(self.nn.layers):
                cfg.acts[i] = l.act_id
            cfg.mode = tmode
            cfg.nprobes = nprobes
            cfg.reg_z, cfg.reg_j, cfg.reg_aug = reg_z, reg_j, reg_aug
            cfg.device_id = self.device.index or 0
            cfg.kernel_path = self.compute_mode.kernel_path
            cfg.arith = arith
            h = _Handle(cfg)
            if self.f64 and not h.lib.cnf_f64_supported(h.ptr):   # JVP modes, flows past the LDS limit: the library's own reason
                raise _lib.CnfError(_lib.ERR_UNSUPPORTED, h.lib.cnf_last_error().decode() + " (data_type=torch.float32 runs it in Float32)")
            self._handles[key] = h
        return h

    def _bind_params(self, h: _Handle, ps: torch.Tensor):
        w_off, b_off, n = self.nn.param_offsets()
        if ps.dtype != self.data_type and ps.dtype in (torch.float32, torch.float64):
            raise _DTypeMismatch(f"ps is {ps.dtype} but the flow was built with data_type={self.data_type}: nothing is cast "
                                 f"silently (DimensionMismatch: ps must be a {'Float64' if self.f64 else 'Float32'} vector of length {n})")
        if ps.dtype != self.data_type or ps.dim() != 1 or ps.numel() != n:
            raise ValueError(f"DimensionMismatch: ps must be a {'Float64' if self.f64 else 'Float32'} vector of length {n}")
        if ps.is_cuda and ps.device != self.device:
            raise ValueError(f"ps lives on {ps.device} but this ICNF is bound to {self.device}")
        # skip the repack only for the SAME tensor object at the same version: a data_ptr alone can be a freed
        # tensor's address handed out again by the caching allocator
        key = (ps.data_ptr(), ps._version, str(ps.device))
        same = h.params_ref is not None and h.params_ref() is ps
        if same and h.params_key == key:
            return
        ps_c = self.nn.abi_params(ps).contiguous()
        wo = (C.c_size_t * len(w_off))(*w_off)
        bo = (C.c_size_t * len(b_off))(*b_off)
        set_params = h.lib.cnf_set_params_f64 if self.f64 else h.lib.cnf_set_params   # two independent bindings of the handle
        _lib.check(set_params(h.ptr, _ptr(ps_c), ps_c.numel(), wo, bo, int(ps_c.is_cuda), _stream_ptr(self.device)))
        h.params_key = key
        h.params_ref = weakref.ref(ps)

    def kernel_path(self, mode: Mode) -> int:
        h = self._handle(mode)
        return int(h.lib.cnf_kernel_path(h.ptr))

    def grad_path(self, mode: Mode, B: Optional[int] = None, alg: int = _lib.ALG_TSIT5, on_grid: bool = False) -> int:
        """0: no gradient for this mode; 1: fused reverse-sweep kernel; 2: layer-wise path; 3: cooperative reverse sweep.
        Without `B` the handle's batch-independent hint (cnf_grad_path); with it, the implementation a call of B columns with
        `alg` on uniform steps / on a grid takes (cnf_grad_path_for)."""
        h = self._handle(mode)
        if B is None:
            return int(h.lib.cnf_grad_path(h.ptr))
        return int(h.lib.cnf_grad_path_for(h.ptr, int(B), int(alg), int(on_grid)))

    def grad_form(self, mode: Mode, B: int, alg: int = _lib.ALG_TSIT5, nsteps: int = 40, on_grid: bool = False) -> int:
        """Which form of the cooperative reverse sweep a call takes (cnf_grad_form_for): 0 none, 1 the sweeps that recompute both
        first-order chains, 2 the second form (the forward solve's stage store + the second-order sweep + products over tiles)."""
        h = self._handle(mode)
        return int(h.lib.cnf_grad_form_for(h.ptr, int(B), int(alg), int(nsteps), int(on_grid)))

    def kernel_family(self, mode: Mode, B: Optional[int] = None, whole_solve: bool = True) -> str:
        """Which kernel organisation serves this mode's handle ("per_wave", "coop", "coopx", "layered", "simt"), or - with `B` -
        a call of B columns ("tile_split" for small whole solves of per-wave shapes): cnf_kernel_family / cnf_kernel_family_for."""
        h = self._handle(mode)
        rc = int(h.lib.cnf_kernel_family(h.ptr)) if B is None else int(h.lib.cnf_kernel_family_for(h.ptr, int(B), int(whole_solve)))
        if rc < 0:
            _lib.check(rc)
        return _lib.FAMILY_NAMES[rc]

    def kernel_name(self, mode: Mode) -> str:
        h = self._handle(mode)
        return h.lib.cnf_kernel_name(h.ptr).decode()

    def repack_on_device(self, mode: Mode) -> bool:
        """True when the last parameter binding of this mode's handle was repacked by the device gather
        kernels (no host round trip) — cnf_repack_on_device."""
        h = self._handle(mode)
        rc = int(h.lib.cnf_repack_on_device(h.ptr))
        if rc < 0:
            _lib.check(rc)
        return bool(rc)

    # Lux-layer call (src/core/base_icnf.jl:509-523)
    def __call__(self, xs, ps, st):
        if self.conditioned:
            x, y = xs
            return inference(self, TrainMode(False), x, y, ps, st)[0], st
        return inference(self, TrainMode(False), xs, ps, st)[0], st


# ---------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------
def setup(rng: Optional[torch.Generator], icnf: ICNF):
    """LuxCore.setup + ComponentArray: flat parameter vector of the flow's data_type (glorot-uniform weights,
    zero biases — Lux.Dense defaults; drawn in float64 either way, so a Float32 flow's vector is the rounded Float64 one)
    and an empty state."""
    if icnf.nn.planar is not None:   # (u, w, b): glorot-uniform vectors, zero bias (planar_layer.jl:36-50)
        pl = icnf.nn.planar
        u = (torch.rand(pl.n_out, generator=rng, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / (pl.n_out + 1))
        w = (torch.rand(pl.n_in, generator=rng, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / (pl.n_in + 1))
        b = torch.zeros(1 if pl.use_bias else 0, dtype=torch.float64)
        return torch.cat([u, w, b]).to(icnf.data_type), {}
    parts = []
    for l in icnf.nn.layers:
        lim = math.sqrt(6.0 / (l.n_in + l.n_out))
        W = (torch.rand(l.n_out, l.n_in, generator=rng, dtype=torch.float64) * 2 - 1) * lim
        parts.append(W.t().reshape(-1))  # column-major (out x in)
        parts.append(torch.zeros(l.n_out, dtype=torch.float64))
    return torch.cat(parts).to(icnf.data_type), {}


def _colmajor(a: torch.Tensor, rows: int, name: str, device, dtype=torch.float32) -> torch.Tensor:
    """(rows, B) tensor -> Julia memory layout (B x rows contiguous), on the device."""
    if a.dim() != 2 or a.shape[0] != rows:
        raise ValueError(f"DimensionMismatch: {name} must be ({rows}, B), got {tuple(a.shape)}")
    if a.device != device:
        raise ValueError(f"{name} must live on {device} (got {a.device})")
    return a.to(dtype).t().contiguous()


def _draw_eps(icnf: ICNF, K: int, B: int) -> torch.Tensor:
    """rand!(rng, epsdist, eps) (src/core/base_icnf.jl:258-259): standard normal unless icnf.epsdist says otherwise."""
    shape = (B, K * icnf.D)
    if icnf.epsdist is None:
        return torch.randn(shape, generator=icnf.rng, device=icnf.device, dtype=icnf.data_type)
    if icnf.epsdist == "rademacher":
        r = torch.randint(0, 2, shape, generator=icnf.rng, device=icnf.device)
        return (2 * r - 1).to(icnf.data_type)
    e = icnf.epsdist(icnf.rng, shape, icnf.device)
    if tuple(e.shape) != shape:
        raise ValueError(f"DimensionMismatch: epsdist must return a {shape} tensor")
    return e.to(device=icnf.device, dtype=icnf.data_type).contiguous()


def _split_args(icnf: ICNF, args, what: str):
    """(xs, ps, st) or (xs, ys, ps, st) as in the reference's method table."""
    if icnf.conditioned:
        if len(args) != 4:
            raise TypeError(f"MethodError: {what}(icnf, mode, xs, ys, ps, st) expected for a "
                            "conditioned ICNF")
        return args
    if len(args) != 3:
        raise TypeError(f"MethodError: {what}(icnf, mode, xs, ps, st) expected")
    return args[0], None, args[1], args[2]


# ---------------------------------------------------------------------------------------
# Float64 flows (ICNF(data_type=torch.float64)): the evaluation path on cnf_*_f64 (csrc/cnf_f64.hip)
# ---------------------------------------------------------------------------------------
def _f64_refuse(icnf: ICNF, what: str) -> None:
    """What a Float64 flow does not do, refused on the arguments alone (before any library call)."""
    if icnf.f64:
        raise NotImplementedError(f"{what} is not implemented for data_type=Float64 (the double-precision path evaluates: "
                                  "augmented_f, inference, generate, loss, logpdf, rand); build the flow with "
                                  "data_type=torch.float32 to use it in Float32")


def _f64_check(icnf: ICNF, what: str, differentiable: bool = False) -> int:
    """The solver of a Float64 call (its alg id), or the refusal - before any library call."""
    if differentiable:
        _f64_refuse(icnf, f"{what}(differentiable=True)")
    kw = icnf.sol_kwargs
    alg = kw.get("alg")
    if alg is None or getattr(alg, "alg_id", None) == _lib.ALG_VCABM or kw.get("adaptive", True):
        raise NotImplementedError(f"{what}: a Float64 flow runs fixed-step solves only - sol_kwargs=dict(alg=Tsit5() or RK4(), "
                                  "adaptive=False, nsteps=... or dt=...); adaptive stepping and VCABM() (the default alg) are "
                                  "implemented in Float32 (data_type=torch.float32)")
    return icnf._solver()


def _f64_cols(icnf: ICNF, a: torch.Tensor, rows: int, name: str) -> torch.Tensor:
    """_colmajor for a Float64 flow: a tensor of another precision is a TypeError, never a cast."""
    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64:
        raise _DTypeMismatch(f"{name} is {getattr(a, 'dtype', type(a).__name__)} but the flow was built with "
                             "data_type=torch.float64: convert it explicitly (nothing is cast silently), or use a Float32 flow")
    return _colmajor(a, rows, name, icnf.device, torch.float64)


def _f64_ps(icnf: ICNF, ps) -> None:
    """The precision of `ps`, checked on the arguments alone (ICNF._bind_params checks it again with the shape)."""
    if not isinstance(ps, torch.Tensor) or ps.dtype != torch.float64:
        raise _DTypeMismatch(f"ps is {getattr(ps, 'dtype', type(ps).__name__)} but the flow was built with data_type=torch.float64: "
                             "convert it explicitly (nothing is cast silently), or use a Float32 flow")


def _f64_inputs(icnf: ICNF, mode: Mode, B: int, eps, ys):
    """(eps, ys) of a call of B columns, column-major: the probes drawn in double unless given."""
    K = icnf.nprobes if isinstance(mode, TrainMode) else 1
    if eps is None:
        e = _draw_eps(icnf, K, B)
    else:
        e = _f64_cols(icnf, eps, K * icnf.D, "eps")
        if e.shape[0] != B:
            raise ValueError("DimensionMismatch: eps must have B columns")
    y = _f64_cols(icnf, ys, icnf.nconditions, "ys") if icnf.conditioned else None
    if y is not None and y.shape[0] != B:
        raise ValueError("DimensionMismatch: xs and ys must have the same number of columns")
    return e, y


def _f64_spans(icnf: ICNF, t0: float, t1: float):
    """The solve from t0 to t1 as [(ta, tb, nsteps)] calls of equal steps: one, or - `dt` with a shorter last step - the full
    steps and the tail of the plan fixed_dt_grid computes.  That plan is made from the Float32 values of dt, t0 and t1 (one plan
    for both precisions, and the one the oracle's fixed_dt_grid makes), so this form carries Float32 times; `nsteps` does not."""
    dt = icnf._fixed_dt()
    if dt is None:
        return [(t0, t1, icnf._nsteps(t0, t1))]
    ts = icnf.fixed_dt_grid(t0, t1, dt)
    if len(ts) < 2:
        return []
    if len(ts) >= 3 and abs(abs(ts[-1] - ts[-2]) - abs(ts[1] - ts[0])) > 1e-7 * abs(t1 - t0):
        return [(ts[0], ts[-2], len(ts) - 2), (ts[-2], ts[-1], 1)]
    return [(ts[0], ts[-1], len(ts) - 1)]


def _f64_integrate(icnf: ICNF, h: _Handle, alg: int, u0c: torch.Tensor, e, y, t0: float, t1: float, sp) -> torch.Tensor:
    """cnf_integrate_fixed_f64 over the spans of the plan; (B, S) column-major in and out."""
    B = u0c.shape[0]
    u1 = u0c.clone()
    for ta, tb, n in _f64_spans(icnf, t0, t1):
        _lib.check(h.lib.cnf_integrate_fixed_f64(h.ptr, alg, n, ta, tb, _ptr(u1), _ptr(e), _ptr(y), B, _ptr(u1), sp))   # in place
    return u1


def _inference_f64(icnf: ICNF, mode: Mode, alg: int, xs, ys, ps, eps, return_state: bool, raw: bool):
    _f64_ps(icnf, ps)
    x = _f64_cols(icnf, xs, icnf.nvariables, "xs")
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev, D, nv, B = icnf.device, icnf.D, icnf.nvariables, x.shape[0]
    e, y = _f64_inputs(icnf, mode, B, eps, ys)
    t0, t1 = icnf._steer_tspan(mode)
    sp = _stream_ptr(dev)
    spans = _f64_spans(icnf, t0, t1)
    if len(spans) == 1:
        ta, tb, n = spans[0]
        logp = torch.empty(B, device=dev, dtype=torch.float64)
        regs = torch.empty(3, B, device=dev, dtype=torch.float64)
        uf = torch.empty(B, icnf.S, device=dev, dtype=torch.float64) if (return_state or icnf.basedist is not None) else None
        _lib.check(h.lib.cnf_inference_fixed_f64(h.ptr, alg, n, ta, tb, _ptr(x), _ptr(e), _ptr(y), B, _ptr(logp), _ptr(regs), _ptr(uf), sp))
    else:   # full steps + tail (or an empty span): the state between the calls, the epilogue in torch float64
        u0 = torch.cat([x, torch.zeros(B, icnf.S - nv, device=dev, dtype=torch.float64)], dim=1)
        uf = _f64_integrate(icnf, h, alg, u0, e, y, t0, t1, sp)
        z = uf[:, :D]
        logp = -0.5 * (z * z).sum(dim=1) - 0.5 * D * math.log(2.0 * math.pi) - uf[:, D]
        reg = isinstance(mode, TrainMode) and mode.reg
        A = torch.sqrt((z[:, nv:] * z[:, nv:]).sum(dim=1)) if (reg and icnf.lambda3 != 0.0 and icnf.augmented) else torch.zeros_like(logp)
        regs = torch.stack([uf[:, D + 1], uf[:, D + 2], A])
    if icnf.basedist is not None:
        logp = icnf.basedist.log_prob(uf[:, :D]).to(torch.float64) - uf[:, D]
    if raw:
        return logp, regs
    out = (logp, (regs[0], regs[1], regs[2]))
    return out + (uf.t(),) if return_state else out


def _generate_f64(icnf: ICNF, mode: Mode, alg: int, ys, ps, n: int, z0, eps):
    dev, D, S = icnf.device, icnf.D, icnf.S
    _f64_ps(icnf, ps)
    if z0 is not None:
        z = _f64_cols(icnf, z0, D, "z0")
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    if z0 is None and icnf.basedist is not None:
        z = icnf.basedist.sample((n,)).to(device=dev, dtype=torch.float64).reshape(n, D)
    elif z0 is None:
        z = torch.randn(n, D, generator=icnf.rng, device=dev, dtype=torch.float64)
    e, y = _f64_inputs(icnf, mode, n, eps, ys)
    u0 = torch.zeros(n, S, device=dev, dtype=torch.float64)
    u0[:, :D] = z
    t0, t1 = icnf._steer_tspan(mode)
    u1 = _f64_integrate(icnf, h, alg, u0, e, y, t1, t0, _stream_ptr(dev))
    return u1[:, :icnf.nvariables].t()


def _augmented_f_f64(icnf: ICNF, mode: Mode, u, ps, t: float, eps, ys):
    _f64_ps(icnf, ps)
    um = _f64_cols(icnf, u, icnf.S, "u")
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    K = icnf.nprobes if isinstance(mode, TrainMode) else 1
    e = None if eps is None else _f64_cols(icnf, eps, K * icnf.D, "eps")
    y = _f64_cols(icnf, ys, icnf.nconditions, "ys") if icnf.conditioned else None
    du = torch.empty_like(um)
    _lib.check(h.lib.cnf_aug_f_f64(h.ptr, _ptr(du), _ptr(um), float(t), _ptr(e), _ptr(y), um.shape[0], _stream_ptr(icnf.device)))
    return du.t()


# ---------------------------------------------------------------------------------------
# the solve as an autograd node (cnf_integrate_fixed_vjp / cnf_integrate_grid_vjp)
# ---------------------------------------------------------------------------------------
def vjp_path(icnf: ICNF, mode: Mode, B: int, alg: int = _lib.ALG_TSIT5, on_grid: bool = False) -> int:
    """Which implementation the pullback of the solve takes for this mode's handle (cnf_vjp_path_for): 1 the fused per-wave
    sweep in its cotangent form, 2 the layer-wise sweep, 0 none."""
    h = icnf._handle(mode)
    return int(h.lib.cnf_vjp_path_for(h.ptr, int(B), int(alg), int(on_grid)))


def _vjp_call(icnf: ICNF, h: _Handle, ps: torch.Tensor, u0c, e, y, alg: int, t0: float, t1: float, nsteps: int, tgrid, u1_bar_c,
              want_u0_bar: bool = True, want_u1: bool = False, want_ys_bar: bool = False):
    """One library call on column-major (B, S) tensors: (gradient in ps's own layout, u0_bar or None, u1 or None) - with
    `want_ys_bar` (conditioned flows; the *_vjp_cond entries) also ys_bar, column-major (B, nconditions), as a fourth item."""
    dev = icnf.device
    B = u0c.shape[0]
    n_abi = ps.numel() if icnf.nn.planar is None else icnf.nn.abi_params(ps).numel()
    grad = torch.empty(n_abi, device=dev, dtype=torch.float32)
    u0_bar = torch.empty_like(u0c) if want_u0_bar else None
    u1 = torch.empty_like(u0c) if want_u1 else None
    sp = _stream_ptr(dev)
    if want_ys_bar:
        ys_bar = torch.empty_like(y)
        if tgrid is not None:
            grid = (C.c_float * len(tgrid))(*tgrid)
            _lib.check(h.lib.cnf_integrate_grid_vjp_cond(h.ptr, alg, len(tgrid) - 1, grid, _ptr(u0c), _ptr(e), _ptr(y), B, _ptr(u1_bar_c),
                                                         _ptr(grad), _ptr(u0_bar), _ptr(ys_bar), _ptr(u1), sp))
        else:
            _lib.check(h.lib.cnf_integrate_fixed_vjp_cond(h.ptr, alg, nsteps, t0, t1, _ptr(u0c), _ptr(e), _ptr(y), B, _ptr(u1_bar_c),
                                                          _ptr(grad), _ptr(u0_bar), _ptr(ys_bar), _ptr(u1), sp))
        return grad[:ps.numel()], u0_bar, u1, ys_bar
    if tgrid is not None:
        grid = (C.c_float * len(tgrid))(*tgrid)
        _lib.check(h.lib.cnf_integrate_grid_vjp(h.ptr, alg, len(tgrid) - 1, grid, _ptr(u0c), _ptr(e), _ptr(y), B, _ptr(u1_bar_c),
                                                _ptr(grad), _ptr(u0_bar), _ptr(u1), sp))
    else:
        _lib.check(h.lib.cnf_integrate_fixed_vjp(h.ptr, alg, nsteps, t0, t1, _ptr(u0c), _ptr(e), _ptr(y), B, _ptr(u1_bar_c),
                                                 _ptr(grad), _ptr(u0_bar), _ptr(u1), sp))
    return grad[:ps.numel()], u0_bar, u1


def integrate_vjp(icnf: ICNF, mode: Mode, u0: torch.Tensor, ps: torch.Tensor, u1_bar: torch.Tensor, *, t0: float, t1: float,
                  eps: Optional[torch.Tensor], ys: Optional[torch.Tensor] = None, tgrid: Optional[Sequence[float]] = None,
                  want_ys_bar: bool = False):
    """The pullback of the fixed-step solve u1 = integrate(u0; ps) - what the reference's ZygoteVJP pullback of `solve` returns
    (src/core/icnf.jl:90-99): for a cotangent `u1_bar` ((S, B)) of the final state, `(grad_ps, u0_bar, u1)` with
    `grad_ps = u1_bar^T du1/dps`, `u0_bar = u1_bar^T du1/du0` ((S, B)) and the forward result `u1`.  The steps are those of
    `sol_kwargs` (`nsteps`, or `dt` with the tail step of the fixed-dt plan) from t0 to t1 - t1 < t0 integrates backwards as
    `generate` does - or the times of `tgrid`.  `eps` ((K*D, B)) are the Hutchinson probes of the solve (ignored in TestMode).
    A shard's `grad_ps` is the partial sum over its columns.
    `want_ys_bar=True` (conditioned flows): `(grad_ps, u0_bar, ys_bar, u1)` with `ys_bar = u1_bar^T du1/dys` ((nconditions, B)),
    the cotangent of the conditions - per column, so a shard's `ys_bar` is complete for its columns."""
    _f64_refuse(icnf, "integrate_vjp (the pullback of the solve)")
    if want_ys_bar and not icnf.conditioned:
        raise ValueError("integrate_vjp(want_ys_bar=True): the flow has no conditions (nconditions = 0)")
    if icnf._solver() == _lib.ALG_VCABM:
        raise NotImplementedError("integrate_vjp: VCABM has no one-step discrete adjoint; use Tsit5 or RK4 (the pullback of a "
                                  "frozen adaptive grid is the `tgrid` argument)")
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev = icnf.device
    u0c = _colmajor(u0, icnf.S, "u0", dev)
    ubc = _colmajor(u1_bar, icnf.S, "u1_bar", dev)
    B = u0c.shape[0]
    if ubc.shape[0] != B:
        raise ValueError("DimensionMismatch: u0 and u1_bar must have the same number of columns")
    K = icnf.nprobes if isinstance(mode, TrainMode) else 1
    e = None if eps is None else _colmajor(eps, K * icnf.D, "eps", dev)
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    grid, nsteps = _fixed_plan(icnf, t0, t1) if tgrid is None else ([float(t) for t in tgrid], 0)
    if want_ys_bar:
        if y.shape[0] != B:
            raise ValueError("DimensionMismatch: u0 and ys must have the same number of columns")
        g, u0_bar, u1, ys_bar = _vjp_call(icnf, h, ps, u0c, e, y, icnf._solver(), t0, t1, nsteps, grid, ubc, True, True, True)
        return g, u0_bar.t(), ys_bar.t(), u1.t()
    g, u0_bar, u1 = _vjp_call(icnf, h, ps, u0c, e, y, icnf._solver(), t0, t1, nsteps, grid, ubc, True, True)
    return g, u0_bar.t(), u1.t()


def _fixed_plan(icnf: ICNF, t0: float, t1: float):
    """(grid or None, nsteps) of a fixed-step solve from t0 to t1 under icnf.sol_kwargs, as loss_and_gradient plans it: equal
    steps, or - fixed dt with a shorter last step - the grid of cnf_integrate_fixed_dt."""
    dt = icnf._fixed_dt()
    ts = icnf.fixed_dt_grid(t0, t1, dt) if dt is not None else None
    if ts is not None and len(ts) >= 2 and abs(abs(ts[-1] - ts[-2]) - abs(ts[1] - ts[0])) > 1e-7 * abs(t1 - t0):
        return ts, len(ts) - 1
    return None, ((len(ts) - 1) if ts is not None and len(ts) >= 2 else icnf._nsteps(t0, t1))


class _Solve(torch.autograd.Function):
    """u1 = integrate(u0; ps) on column-major (B, S) states.  The forward is the library's plain solve; the backward is one
    cnf_integrate_*_vjp call on the current stream, on the steps the forward took (an adaptive Tsit5 solve: its accepted steps,
    frozen).  Nothing is kept in the library's handle between the two.  The conditions `y` ((B, nconditions), column-major) are
    a differentiable input when they require grad (cond_grad=True): the backward is then the *_vjp_cond call and returns ys_bar."""

    @staticmethod
    def forward(ctx, u0c, ps, icnf, mode, e, y, t0, t1, group):
        h = icnf._handle(mode)
        icnf._bind_params(h, ps)
        dev = icnf.device
        B = u0c.shape[0]
        alg = icnf._solver()
        u0c = u0c.contiguous()
        if icnf.adaptive:
            u1 = _adaptive_integrate(icnf, h, u0c, t0, t1, e, y, group=group, _tsit5=True)
            ts = [t0]
            for d in icnf.last_solve_stats["dts"]:
                ts.append(ts[-1] + d)
            ts[-1] = t1
            icnf.last_solve_stats["tgrid"] = ts
            grid, nsteps, alg = ts, len(ts) - 1, _lib.ALG_TSIT5
        else:
            grid, nsteps = _fixed_plan(icnf, t0, t1)
            u1 = torch.empty_like(u0c)
            dt = icnf._fixed_dt()
            if dt is not None:
                _lib.check(h.lib.cnf_integrate_fixed_dt(h.ptr, alg, dt, t0, t1, _ptr(u0c), _ptr(e), _ptr(y), B, _ptr(u1), _stream_ptr(dev)))
            else:
                _lib.check(h.lib.cnf_integrate_fixed(h.ptr, alg, nsteps, t0, t1, _ptr(u0c), _ptr(e), _ptr(y), B, _ptr(u1), _stream_ptr(dev)))
        ctx.save_for_backward(u0c, ps)
        ctx.rest = (icnf, mode, e, y, alg, t0, t1, nsteps, grid)
        return u1

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, u1_bar):
        u0c, ps = ctx.saved_tensors
        icnf, mode, e, y, alg, t0, t1, nsteps, grid = ctx.rest
        h = icnf._handle(mode)
        icnf._bind_params(h, ps)
        if y is not None and ctx.needs_input_grad[5]:
            g, u0_bar, _, ys_bar = _vjp_call(icnf, h, ps, u0c, e, y, alg, t0, t1, nsteps, grid, u1_bar.contiguous().to(torch.float32),
                                             ctx.needs_input_grad[0], False, True)
            return u0_bar, (g if ctx.needs_input_grad[1] else None), None, None, None, ys_bar, None, None, None
        g, u0_bar, _ = _vjp_call(icnf, h, ps, u0c, e, y, alg, t0, t1, nsteps, grid, u1_bar.contiguous().to(torch.float32),
                                 ctx.needs_input_grad[0], False)
        return u0_bar, (g if ctx.needs_input_grad[1] else None), None, None, None, None, None, None, None


def _check_differentiable(icnf: ICNF, ys, what: str, cond_grad: bool = False):
    if icnf._solver() == _lib.ALG_VCABM:
        raise NotImplementedError(f"{what}(differentiable=True): VCABM has no one-step discrete adjoint here; use "
                                  "sol_kwargs alg=Tsit5() (adaptive or fixed-step) or RK4(), or loss_and_gradient, which "
                                  "differentiates the adaptive Tsit5 discretisation instead")
    if not cond_grad and ys is not None and getattr(ys, "requires_grad", False):
        raise NotImplementedError(f"{what}(differentiable=True): no gradient with respect to ys; pass ys.detach() "
                                  "(the conditions enter the solve as constants), or cond_grad=True to differentiate with "
                                  "respect to them")


def _check_cond_grad(icnf: ICNF, differentiable: bool, cond_grad: bool, what: str):
    """cond_grad=True needs differentiable=True and a conditioned flow: refused before any library call."""
    if not cond_grad:
        return
    if not differentiable:
        raise ValueError(f"{what}(cond_grad=True) needs differentiable=True")
    if not icnf.conditioned:
        raise ValueError(f"{what}(cond_grad=True): the flow has no conditions (nconditions = 0)")


def _inference_differentiable(icnf: ICNF, mode: Mode, xs, ys, ps, eps, return_state: bool, group, cond_grad: bool = False):
    """inference with the solve as an autograd node and the epilogue in plain torch: logp, E, n, A (and the state) carry
    gradients to ps and xs - and, with cond_grad, to ys."""
    _check_differentiable(icnf, ys, "inference", cond_grad)
    dev = icnf.device
    D, nv = icnf.D, icnf.nvariables
    if xs.dim() != 2 or xs.shape[0] != nv:
        raise ValueError(f"DimensionMismatch: xs must be ({nv}, B), got {tuple(xs.shape)}")
    if xs.device != dev:
        raise ValueError(f"xs must live on {dev} (got {xs.device})")
    B = xs.shape[1]
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    if y is not None and y.shape[0] != B:
        raise ValueError("DimensionMismatch: xs and ys must have the same number of columns")
    K = icnf.nprobes if isinstance(mode, TrainMode) else 1
    if eps is None:
        e = _draw_eps(icnf, K, B)     # drawn once per call; the backward reuses it
    else:
        e = _colmajor(eps, K * D, "eps", dev)
        if e.shape[0] != B:
            raise ValueError("DimensionMismatch: eps must have B columns")
    t0, t1 = icnf._steer_tspan(mode)
    u0c = torch.cat([xs.to(torch.float32).t(), torch.zeros(B, icnf.S - nv, device=dev, dtype=torch.float32)], dim=1)
    uf = _Solve.apply(u0c, ps, icnf, mode, e, y, t0, t1, group)
    z = uf[:, :D]
    if icnf.basedist is not None:
        logp = icnf.basedist.log_prob(z).to(torch.float32) - uf[:, D]
    else:
        logp = -0.5 * (z * z).sum(dim=1) - 0.5 * D * math.log(2.0 * math.pi) - uf[:, D]
    reg = isinstance(mode, TrainMode) and mode.reg
    if reg and icnf.lambda3 != 0.0 and icnf.augmented:   # A = |z_aug| (src/core/base_icnf.jl:106-122)
        A = torch.sqrt((z[:, nv:] * z[:, nv:]).sum(dim=1))
    else:
        A = torch.zeros(B, device=dev, dtype=torch.float32)
    out = (logp, (uf[:, D + 1], uf[:, D + 2], A))
    if return_state:
        return out + (uf.t(),)
    return out


def inference(icnf: ICNF, mode: Mode, *args, eps: Optional[torch.Tensor] = None,
              return_state: bool = False, _raw: bool = False, group=None, _sp=None, differentiable: bool = False,
              cond_grad: bool = False):
    """inference(icnf, mode, xs[, ys], ps, st) -> (logp̂x (B,), (Ė, ṅ, Ȧ)).

    `eps` ((K*D, B)) pins the Hutchinson probes; by default they are drawn from icnf.rng as
    the reference does.  xs is (nvariables, B), ys (nconditions, B).
    `group`: under an ADAPTIVE solver the error norm couples all columns, so when the batch is sharded over ranks the
    solve all-reduces its error sums over `group` (None = the default group / the installed Comm) and every rank must
    make this call; `group=False` (or `icnf.sharded = False`) runs a rank-local solve with no collectives.  Fixed-step
    solves never communicate.
    `differentiable=True`: the solve is a torch.autograd node (its backward is the library's pullback of the solve,
    cnf_integrate_*_vjp) and the epilogue - log N(z) or `icnf.basedist.log_prob(z)`, minus dlogp; A = |z_aug| - is plain torch,
    so logp, E, n, A and the returned state carry gradients to `ps` and `xs`: any scalar built on them can be differentiated
    (sample weights, another base distribution, a logsumexp over flows).  Under an adaptive Tsit5 solver the backward runs on
    the steps the forward accepted.  Not with VCABM.  With respect to `ys` only when `cond_grad=True` is given as well (a
    conditioned flow whose conditions come from an encoder trained jointly with it): the backward then also returns the cotangent
    of the conditions (cnf_integrate_*_vjp_cond); without it a `ys` that requires grad is refused.  Each rank's gradient is the
    partial sum of its own columns (the gradient of `ys` is per column)."""
    xs, ys, ps, st = _split_args(icnf, args, "inference")
    _check_cond_grad(icnf, differentiable, cond_grad, "inference")
    if icnf.f64:
        return _inference_f64(icnf, mode, _f64_check(icnf, "inference", differentiable), xs, ys, ps, eps, return_state, _raw)
    group = icnf._group(group)
    if differentiable:
        return _inference_differentiable(icnf, mode, xs, ys, ps, eps, return_state, group, cond_grad)
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev = icnf.device
    x = _colmajor(xs, icnf.nvariables, "xs", dev)
    B = x.shape[0]
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    if y is not None and y.shape[0] != B:
        raise ValueError("DimensionMismatch: xs and ys must have the same number of columns")
    train = isinstance(mode, TrainMode)
    K = icnf.nprobes if train else 1
    if eps is None:
        e = _draw_eps(icnf, K, B)  # drawn (and unused) in TestMode too, like base_icnf.jl:258
    else:
        e = _colmajor(eps, K * icnf.D, "eps", dev)
        if e.shape[0] != B:
            raise ValueError("DimensionMismatch: eps must have B columns")
    t0, t1 = icnf._steer_tspan(mode)
    alg = icnf._solver()
    logp = torch.empty(B, device=dev, dtype=torch.float32)
    regs = torch.empty(3, B, device=dev, dtype=torch.float32)
    want_state = return_state or icnf.basedist is not None
    sp = _sp if _sp is not None else _stream_ptr(dev)   # torch's current stream, looked up once per call (5 us a lookup; a small-batch solve is 200)
    if icnf.adaptive:
        u0 = torch.empty(B, icnf.S, device=dev, dtype=torch.float32)
        if B:
            _lib.check(h.lib.cnf_assemble_u0(h.ptr, _ptr(x), B, _ptr(u0), sp))
        uf = _adaptive_integrate(icnf, h, u0, t0, t1, e, y, group=group, _sp=sp)
        if B:
            _lib.check(h.lib.cnf_epilogue(h.ptr, _ptr(uf), B, _ptr(logp), _ptr(regs), sp))
    else:
        uf = torch.empty(B, icnf.S, device=dev, dtype=torch.float32) if want_state else None
        dt = icnf._fixed_dt()
        if dt is not None:
            _lib.check(h.lib.cnf_inference_fixed_dt(h.ptr, alg, dt, t0, t1, _ptr(x), _ptr(e), _ptr(y), B,
                                                    _ptr(logp), _ptr(regs), _ptr(uf), sp))
        else:
            _lib.check(h.lib.cnf_inference_fixed(h.ptr, alg, icnf._nsteps(t0, t1), t0, t1, _ptr(x), _ptr(e), _ptr(y), B,
                                                 _ptr(logp), _ptr(regs), _ptr(uf), sp))
    if icnf.basedist is not None:   # logp̂x = logpdf(basedist, z) - Δlogp (base_icnf.jl:168-169)
        logp = (icnf.basedist.log_prob(uf[:, :icnf.D]) - uf[:, icnf.D]).to(torch.float32)
    if _raw:   # internal: the (3, B) regulariser block as one tensor (no copies on the loss path)
        return logp, regs
    out = (logp, (regs[0], regs[1], regs[2]))
    if return_state:
        return out + (uf.t(),)
    return out


def generate(icnf: ICNF, mode: Mode, *args, z0: Optional[torch.Tensor] = None,
             eps: Optional[torch.Tensor] = None, group=None, differentiable: bool = False, cond_grad: bool = False):
    """generate(icnf, mode, [ys,] ps, st, n) -> (nvariables, n) samples: integrate the base
    sample backwards over the reversed tspan (src/core/base_icnf.jl:351-404, 185-194).
    `differentiable=True`: the solve is a torch.autograd node (see `inference`), so the samples carry gradients to `ps` and to
    `z0` - training on generated samples (reverse KL) - and, with `cond_grad=True` on a conditioned flow, to `ys`."""
    _check_cond_grad(icnf, differentiable, cond_grad, "generate")
    if icnf.conditioned:
        if len(args) != 4:
            raise TypeError("MethodError: generate(icnf, mode, ys, ps, st, n) expected")
        ys, ps, st, n = args
    else:
        if len(args) != 3:
            raise TypeError("MethodError: generate(icnf, mode, ps, st, n) expected")
        ps, st, n = args
        ys = None
    if icnf.f64:
        return _generate_f64(icnf, mode, _f64_check(icnf, "generate", differentiable), ys, ps, n, z0, eps)
    if differentiable:
        _check_differentiable(icnf, ys, "generate", cond_grad)
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev = icnf.device
    D, S = icnf.D, icnf.S
    if z0 is None and icnf.basedist is not None:
        z = icnf.basedist.sample((n,)).to(device=dev, dtype=torch.float32).reshape(n, D)
    elif z0 is None:
        z = torch.randn(n, D, generator=icnf.rng, device=dev, dtype=torch.float32)
    else:
        z = _colmajor(z0, D, "z0", dev)
    train = isinstance(mode, TrainMode)
    K = icnf.nprobes if train else 1
    e = _draw_eps(icnf, K, n) if eps is None else _colmajor(eps, K * D, "eps", dev)
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    u0 = torch.zeros(n, S, device=dev, dtype=torch.float32)
    u0[:, :D] = z
    t0, t1 = icnf._steer_tspan(mode)
    if differentiable:
        if z.requires_grad:   # (z0 given with a graph: the state is assembled by torch so the cotangent reaches it)
            u0 = torch.cat([z, torch.zeros(n, S - D, device=dev, dtype=torch.float32)], dim=1)
        u1 = _Solve.apply(u0, ps, icnf, mode, e, y, t1, t0, icnf._group(group))
        return u1[:, :icnf.nvariables].t()
    alg = icnf._solver()
    if icnf.adaptive:
        u1 = _adaptive_integrate(icnf, h, u0, t1, t0, e, y, group=icnf._group(group))
    else:
        u1 = torch.empty_like(u0)
        dt = icnf._fixed_dt()
        if dt is not None:
            _lib.check(h.lib.cnf_integrate_fixed_dt(h.ptr, alg, dt, t1, t0, _ptr(u0), _ptr(e), _ptr(y), n,
                                                    _ptr(u1), _stream_ptr(dev)))
        else:
            _lib.check(h.lib.cnf_integrate_fixed(h.ptr, alg, icnf._nsteps(t0, t1), t1, t0, _ptr(u0), _ptr(e), _ptr(y), n,
                                                 _ptr(u1), _stream_ptr(dev)))
    return u1[:, :icnf.nvariables].t()


def augmented_f(icnf: ICNF, mode: Mode, u: torch.Tensor, ps: torch.Tensor, t: float,
                eps: Optional[torch.Tensor], ys: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One dynamics call du = f(u, p, t): the closure of make_ode_func
    (src/core/base_icnf.jl:62-78; src/core/icnf.jl:517-536).  u: (S, B)."""
    if icnf.f64:
        return _augmented_f_f64(icnf, mode, u, ps, t, eps, ys)
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev = icnf.device
    um = _colmajor(u, icnf.S, "u", dev)
    B = um.shape[0]
    train = isinstance(mode, TrainMode)
    K = icnf.nprobes if train else 1
    e = None if eps is None else _colmajor(eps, K * icnf.D, "eps", dev)
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    du = torch.empty_like(um)
    _lib.check(h.lib.cnf_aug_f(h.ptr, _ptr(du), _ptr(um), float(t), _ptr(e), _ptr(y), B,
                               _stream_ptr(dev)))
    return du.t()


def loss_sums(icnf: ICNF, mode: Mode, logp: torch.Tensor, regs) -> torch.Tensor:
    """Device-side partial sums [Σ-logp, ΣĖ, Σṅ, ΣȦ] of this rank's columns."""
    h = icnf._handle(mode)
    B = logp.numel()
    r = torch.stack(list(regs)).contiguous() if not (
        isinstance(regs, torch.Tensor) and regs.is_contiguous()) else regs
    sums = torch.zeros(4, device=icnf.device, dtype=torch.float32)
    if B:
        _lib.check(h.lib.cnf_loss_sums(h.ptr, _ptr(logp.contiguous()), _ptr(r), B, _ptr(sums),
                                       _stream_ptr(icnf.device)))
    return sums


def loss_mean(icnf: ICNF, mode: Mode, logp: torch.Tensor, regs, _sp=None) -> torch.Tensor:
    """The scalar loss of an UNSHARDED batch from (logp, regs) in the library's two reduction kernels
    (`cnf_loss_mean`): mean(-logp + λ₁Ė + λ₂ṅ + λ₃Ȧ), combined in float64, returned as a 0-dim float32 tensor."""
    import ctypes as C
    h = icnf._handle(mode)
    B = logp.numel()
    if B == 0:
        return torch.full((), float("nan"), device=icnf.device, dtype=torch.float32)
    r = torch.stack(list(regs)).contiguous() if not (
        isinstance(regs, torch.Tensor) and regs.is_contiguous()) else regs
    out = torch.empty(1, device=icnf.device, dtype=torch.float32)
    lam = (C.c_double * 3)(float(icnf.lambda1), float(icnf.lambda2), float(icnf.lambda3))
    _lib.check(h.lib.cnf_loss_mean(h.ptr, _ptr(logp.contiguous()), _ptr(r), B, lam, None, _ptr(out),
                                   _sp if _sp is not None else _stream_ptr(icnf.device)))
    return out[0]


def _loss_adaptive_one_call(icnf: ICNF, mode: Mode, args, eps, sp):
    """`loss` of an unsharded batch under an adaptive solver as ONE library call (cnf_loss_adaptive: u0 assembly, the VCABM or
    adaptive Tsit5 solve, the epilogue, the mean - the same kernels `inference` + `loss_mean` enqueue, so the same bits).  What it
    saves is host time: at the reference's own batch size (2^10 samples, its PkgBenchmark suite) a solve is ~0.13 ms of kernel and
    the Python / ctypes side of four calls another ~0.03.  Returns None for an empty batch (the general path raises / returns NaN)."""
    xs, ys, ps, st = _split_args(icnf, args, "loss")
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev = icnf.device
    x = _colmajor(xs, icnf.nvariables, "xs", dev)
    B = x.shape[0]
    if B == 0:
        return None
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    if y is not None and y.shape[0] != B:
        raise ValueError("DimensionMismatch: xs and ys must have the same number of columns")
    K = icnf.nprobes if isinstance(mode, TrainMode) else 1
    if eps is None:
        e = _draw_eps(icnf, K, B)
    else:
        e = _colmajor(eps, K * icnf.D, "eps", dev)
        if e.shape[0] != B:
            raise ValueError("DimensionMismatch: eps must have B columns")
    t0, t1 = icnf._steer_tspan(mode)
    kw = icnf.sol_kwargs
    vcabm = icnf._solver() == _lib.ALG_VCABM
    cap = 4096
    rec = getattr(icnf, "_loss_records", None)
    if rec is None:
        rec = icnf._loss_records = (_lib.SolveStats(), (C.c_float * cap)(), (C.c_int32 * cap)(), (C.c_double * 3)())
    ss, dts, orders, lam = rec
    lam[0], lam[1], lam[2] = float(icnf.lambda1), float(icnf.lambda2), float(icnf.lambda3)
    out = torch.empty(1, device=dev, dtype=torch.float32)
    _solve_errors(lambda: h.lib.cnf_loss_adaptive(
        h.ptr, _lib.ALG_VCABM if vcabm else _lib.ALG_TSIT5, t0, t1, _ptr(x), _ptr(e), _ptr(y), B, float(kw.get("abstol", 1e-4)),
        float(kw.get("reltol", 1e-4)), float(kw["dt"]) if "dt" in kw else 0.0, _lib.clamp_maxiters(kw), lam, _ptr(out), None, None, None,
        C.byref(ss), dts, orders, cap, sp))
    m = min(ss.naccept, cap)
    stats = {"naccept": ss.naccept, "nreject": ss.nreject, "nf": ss.nf, "dts": [float(v) for v in dts[:m]],
             "alg_used": "VCABM" if vcabm else "Tsit5", "controller": "device" if h.lib.cnf_solve_controller(h.ptr) == 1 else "host"}
    if vcabm:
        stats["orders"] = [int(v) for v in orders[:m]]
    icnf.last_solve_stats = stats
    return out[0]


def loss(icnf: ICNF, mode: Mode, *args, eps: Optional[torch.Tensor] = None, group=None):
    """loss(icnf, mode, xs[, ys], ps, st) = mean(-logp̂x + λ₁Ė + λ₂ṅ + λ₃Ȧ)
    (src/core/icnf.jl:628-649).  When torch.distributed is initialised the batch columns are
    taken to be sharded over the ranks of `group`: the four partial sums and the column count
    are all-reduced (RCCL over xGMI on GPUs) and every rank returns the global mean."""
    from .sharding import reduce_loss
    group = icnf._group(group)
    from .sharding import is_sharded
    if icnf.f64:   # the mean in torch float64; a sharded mean in double is not provided
        _f64_check(icnf, "loss")
        if is_sharded(group):
            _f64_refuse(icnf, "loss over column shards")
        logp, regs = inference(icnf, mode, *args, eps=eps, _raw=True)
        return (-logp + icnf.lambda1 * regs[0] + icnf.lambda2 * regs[1] + icnf.lambda3 * regs[2]).mean()
    sp = _stream_ptr(icnf.device)
    if (icnf.adaptive and not is_sharded(group) and icnf.basedist is None and getattr(icnf, "adaptive_policy", "library") == "library"):
        out = _loss_adaptive_one_call(icnf, mode, args, eps, sp)
        if out is not None:
            return out
    logp, regs = inference(icnf, mode, *args, eps=eps, _raw=True, group=group, _sp=sp)
    if not is_sharded(group) and logp.numel():
        return loss_mean(icnf, mode, logp, regs, _sp=sp)       # one process: the mean comes out of the reduction kernels themselves
    sums = loss_sums(icnf, mode, logp, regs)
    return reduce_loss(sums, logp.numel(), (icnf.lambda1, icnf.lambda2, icnf.lambda3), group=group)


def loss_and_gradient(icnf: ICNF, mode: Mode, *args, eps: Optional[torch.Tensor] = None, group=None,
                      wrt_x: bool = False):
    """(loss, dloss/dps) for `loss(icnf, mode, xs, ps, st)` — what `Zygote.gradient` of the
    reference's training objective returns (src/exts/mlj_ext/core_icnf.jl:42-51), here the exact
    gradient of the discrete fixed-step loss, computed by the reverse-sweep HIP kernel.  With
    torch.distributed initialised the column shards' gradients (nparams floats) and loss sums are
    all-reduced (RCCL over xGMI) and every rank returns the global mean and its gradient.
    `wrt_x=True` also returns dloss/dxs, (nvariables, B) for this rank's columns (`DI.gradient` with respect
    to the data in test/ci_tests/smoke_tests.jl): the costate at t0, a by-product of the same sweep.

    Solver substitution (recorded in `icnf.last_solve_stats["alg_used"]` / `["gradient_of"]`): with a fixed-step
    solver the value and gradient are those of exactly the discretisation `loss()` evaluates.  With an ADAPTIVE solver
    the accepted steps of an adaptive *Tsit5* solve are frozen and the discrete solve on that grid is reversed — also
    when `sol_kwargs.alg` is VCABM (the reference's default), whose multistep recurrence has no one-step discrete
    adjoint here.  So under VCABM the returned value is the Tsit5-grid loss, which agrees with `loss()` (VCABM) only
    to the solver tolerance (tests/test_parity_gpu.py bounds the difference); the reference's own gradient
    (QuadratureAdjoint, icnf.jl:90-99) is likewise a separate solve that matches its forward pass to tolerance."""
    from .sharding import global_count, is_sharded, reduce_gradient, reduce_loss
    _f64_refuse(icnf, "loss_and_gradient")
    group = icnf._group(group)
    xs, ys, ps, st = _split_args(icnf, args, "loss_and_gradient")
    if icnf.basedist is not None:
        raise NotImplementedError("loss_and_gradient: the terminal costate assumes basedist = MvNormal(0, I)")
    h = icnf._handle(mode)
    icnf._bind_params(h, ps)
    dev = icnf.device
    x = _colmajor(xs, icnf.nvariables, "xs", dev)
    B = x.shape[0]
    y = _colmajor(ys, icnf.nconditions, "ys", dev) if icnf.conditioned else None
    K = icnf.nprobes if isinstance(mode, TrainMode) else 1      # as `inference`: TestMode ignores the probes
    e = _draw_eps(icnf, K, B) if eps is None else _colmajor(eps, K * icnf.D, "eps", dev)
    t0, t1 = icnf._steer_tspan(mode)
    # the library differentiates with respect to the vector it was given (Chain.abi_params): ps itself, or for a PlanarLayer ps
    # followed by the pinned zero biases, whose gradient entries are dropped below
    n_abi = ps.numel() if icnf.nn.planar is None else icnf.nn.abi_params(ps).numel()
    grad = torch.empty(n_abi, device=dev, dtype=torch.float32)
    gx = torch.zeros(B, icnf.nvariables, device=dev, dtype=torch.float32) if wrt_x else None
    sums = torch.empty(4, device=dev, dtype=torch.float32)
    lam = (C.c_float * 3)(icnf.lambda1, icnf.lambda2, icnf.lambda3)
    if icnf.adaptive and not is_sharded(group) and getattr(icnf, "adaptive_policy", "library") == "library":
        # single process: adaptive Tsit5 solve + frozen-grid gradient in one library call (cnf_loss_grad_adaptive)
        kw = icnf.sol_kwargs
        cap = 4096
        ss, tg = _lib.SolveStats(), (C.c_float * cap)()
        _solve_errors(lambda: h.lib.cnf_loss_grad_adaptive(
            h.ptr, t0, t1, _ptr(x), _ptr(e), _ptr(y), B, float(kw.get("abstol", 1e-4)), float(kw.get("reltol", 1e-4)),
            float(kw["dt"]) if "dt" in kw else 0.0, _lib.clamp_maxiters(kw), lam, _ptr(grad), _ptr(gx), _ptr(sums),
            C.byref(ss), tg, cap, _stream_ptr(dev)))
        ts = [float(v) for v in tg[:min(ss.naccept + 1, cap)]]
        icnf.last_solve_stats = {"naccept": ss.naccept, "nreject": ss.nreject, "nf": ss.nf, "tgrid": ts,
                                 "dts": [b - a for a, b in zip(ts, ts[1:])], "alg_used": "Tsit5",
                                 "gradient_of": "adaptive Tsit5 solve, accepted steps frozen (discrete adjoint on that grid)"}
    elif icnf.adaptive:
        # differentiate the discrete solve on the steps the adaptive solver accepted (frozen grid; the dependence
        # of the step sizes on ps is ignored - the discretise-then-optimise convention)
        u0 = torch.empty(B, icnf.S, device=dev, dtype=torch.float32)
        _lib.check(h.lib.cnf_assemble_u0(h.ptr, _ptr(x), B, _ptr(u0), _stream_ptr(dev)))
        # (also under VCABM: a multistep recurrence has no one-step discrete adjoint here, so training differentiates
        # the adaptive Tsit5 discretisation at the same tolerances - the reference's own QuadratureAdjoint gradient is
        # likewise a separate solve that matches the forward pass only to tolerance)
        _adaptive_integrate(icnf, h, u0, t0, t1, e, y, group=group, _tsit5=True)
        ts = [t0]
        for d in icnf.last_solve_stats["dts"]:
            ts.append(ts[-1] + d)
        ts[-1] = t1
        grid = (C.c_float * len(ts))(*ts)
        icnf.last_solve_stats["tgrid"] = ts
        icnf.last_solve_stats["gradient_of"] = "adaptive Tsit5 solve, accepted steps frozen (discrete adjoint on that grid)"
        _lib.check(h.lib.cnf_loss_grad_grid(h.ptr, _lib.ALG_TSIT5, len(ts) - 1, grid, _ptr(x), _ptr(e), _ptr(y), B, lam,
                                            _ptr(grad), _ptr(gx), _ptr(sums), _stream_ptr(dev)))
    else:
        icnf.last_solve_stats = {"alg_used": "Tsit5" if icnf._solver() == _lib.ALG_TSIT5 else "RK4",
                                 "gradient_of": "the fixed-step solve loss() evaluates (exact discrete adjoint)"}
        dt = icnf._fixed_dt()
        ts = icnf.fixed_dt_grid(t0, t1, dt) if dt is not None else None
        if ts is not None and len(ts) >= 2 and abs((ts[-1] - ts[-2]) - (ts[1] - ts[0])) > 1e-7 * abs(t1 - t0):
            # fixed dt with a shorter last step (a STEER-drawn t1): the same grid as cnf_inference_fixed_dt, reversed exactly
            grid = (C.c_float * len(ts))(*ts)
            icnf.last_solve_stats["tgrid"] = ts
            _lib.check(h.lib.cnf_loss_grad_grid(h.ptr, icnf._solver(), len(ts) - 1, grid, _ptr(x), _ptr(e), _ptr(y), B, lam,
                                                _ptr(grad), _ptr(gx), _ptr(sums), _stream_ptr(dev)))
        else:
            nsteps = (len(ts) - 1) if ts is not None and len(ts) >= 2 else icnf._nsteps(t0, t1)
            _lib.check(h.lib.cnf_loss_grad_fixed(h.ptr, icnf._solver(), nsteps, t0, t1, _ptr(x), _ptr(e),
                                                 _ptr(y), B, lam, _ptr(grad), _ptr(gx), _ptr(sums), _stream_ptr(dev)))
    value = reduce_loss(sums, B, (icnf.lambda1, icnf.lambda2, icnf.lambda3), group=group)
    gps = reduce_gradient(grad[:ps.numel()], B, group=group)
    if not wrt_x:
        return value, gps
    Bg = global_count(B, dev, group)
    return value, gps, (gx / Bg).t()
