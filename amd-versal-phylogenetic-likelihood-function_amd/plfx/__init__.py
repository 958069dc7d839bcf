"""plfx -- Python binding of libplfx.so (include/plfx.h), the MI355X PLF engine.

The binding mirrors the reference's interfaces for the PLF hot path:

* ``plf(x1_start, x2_start, x3_start, EV, n, left, right, wgt)`` -- the
  reference CPU entry point ``plf()`` (/root/reference/app/src/plf.h:1-5):
  same argument order and meaning; the ``int& scalerIncrement`` out-argument
  becomes the return value.  Runs on the GPU through ``plfx_plf_f32/f64``.
* ``plf_dev(...)`` -- the same update on device-resident torch tensors,
  asynchronous on a HIP stream (``plfx_plf_dev_f32/f64``); optional per-site
  scaler bytes (the s2mm char output, hls/src/s2mm_memDNAwindowComb.cpp:97) and
  weighted scaler sum (host_mem.cpp:384-388).
* ``instance_run(...)`` -- the accelerator instance-buffer contract
  (host_mem.cpp:123-157): packed [EV|P_L|CLV_L] / [EV|P_R|CLV_R] or [P_R|CLV_R].
* ``Testbench`` / ``pack_instance`` -- testbench_info sizing
  (app/src/include.h:150-266) and packing (host_mem.cpp:221-243).

There is no CPU fallback: if libplfx.so or a gfx950 device is missing every
call raises ``PlfxError``.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libplfx.so"

OK = 0
ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_NODEV, ERR_UNSUPPORTED = -1, -2, -3, -4, -5
LAYOUT_COMBINED, LAYOUT_SEPARATE = 0, 1
AIE_STREAM, AIE_WINDOW = 0, 1
F32, F64 = 0, 1

# symbols declared by include/plfx.h (checked by tests/test_abi.py)
EXPORTS = (
    "plfx_ctx_create", "plfx_ctx_create_ex", "plfx_ctx_destroy", "plfx_last_error", "plfx_get_version",
    "plfx_ctx_stream", "plfx_ctx_device", "plfx_ctx_synchronize", "plfx_ctx_release_stream",
    "plfx_ctx_set_streams", "plfx_ctx_streams",
    "plfx_plf_f32", "plfx_plf_f64", "plfx_plf_dev_f32", "plfx_plf_dev_f64",
    "plfx_instance_run", "plfx_instance_run_host", "plfx_scaler_sum",
    "plfx_tb_alignments_per_instance", "plfx_tb_alignments_padding",
    "plfx_tb_instance_site_offset", "plfx_tb_elements_per_instance",
    "plfx_tb_instance_elements_left", "plfx_tb_instance_elements_right",
    "plfx_tb_instance_elements_out",
    "plfx_tb_instance_active_elements_left", "plfx_tb_instance_active_elements_right",
    "plfx_tb_num_windows_per_instance", "plfx_pack_instance",
    "plfx_plf_batch_dev", "plfx_traverse", "plfx_root_lnl", "plfx_plf_dev_gen",
    "plfx_plf_tips_dev", "plfx_plf_tips_dev_gen", "plfx_traverse_tips",
    "plfx_model_eigen", "plfx_gamma_rates", "plfx_model_ev", "plfx_model_root_weights",
    "plfx_pmatrix", "plfx_model_tip_vectors",
    "plfx_shard", "plfx_gen_hostmem", "plfx_swemu_instance_run", "plfx_traverse_schedule",
    "plfx_edge_sumtable", "plfx_edge_derivatives", "plfx_edge_optimize", "plfx_edge_optimize_dev",
    "plfx_plf_psr_dev", "plfx_root_lnl_psr", "plfx_edge_sumtable_psr", "plfx_edge_derivatives_psr",
    "plfx_edge_optimize_psr", "plfx_traverse_psr",
    "plfx_edge_optimize_psr_dev", "plfx_edge_sumtable_psr_batch",
    "plfx_site_lnl_psr", "plfx_psr_rate_scan", "plfx_psr_rate_scan_workspace", "plfx_psr_categorize",
    "plfx_plf_psr_dev_gen", "plfx_traverse_psr_gen", "plfx_root_lnl_psr_gen", "plfx_psr_site_order",
    "plfx_edge_sumtable_psr_gen", "plfx_edge_sumtable_psr_batch_gen", "plfx_edge_derivatives_psr_gen",
    "plfx_edge_optimize_psr_gen", "plfx_edge_optimize_psr_dev_gen",
    "plfx_site_lnl_psr_gen", "plfx_psr_rate_scan_gen", "plfx_psr_rate_scan_workspace_gen",
    "plfx_plf_psr_dev_ex", "plfx_traverse_psr_ex", "plfx_psr_rate_scan_ex",
    "plfx_branch_sumtables_psr", "plfx_branch_sumtables_psr_workspace", "plfx_branch_pair_sites_per_lane",
)
EDGE_MAX_EVALS = 256  # PLFX_EDGE_MAX_EVALS
PSR_MAX_CATS = 32     # PLFX_PSR_MAX_CATS
PSR_SCAN_MAX_RATES = 1024  # PLFX_PSR_SCAN_MAX_RATES
MAX_STREAMS = 64   # PLFX_MAX_STREAMS
WS_POOL = 8        # PLFX_WS_POOL
STREAMS_MAX = 8    # PLFX_STREAMS_MAX
STREAM_PER_THREAD = 2  # hipStreamPerThread
SCHED_KEYS = ("deep6", "deep5", "deep4", "septets", "triples", "unfused", "launches")
PMAT_STATE, PMAT_EIGEN = 0, 1
EXACT, FMA = 0, 1
VALU = 2  # with FMA: protein f64 on the VALU (not the matrix cores): P and EV as wave-uniform scalar
          # operands, LDS holds only the staged child tile
BRANCH_NOFUSE = 4  # PLFX_BRANCH_NOFUSE: branch_sumtables_psr lowers every op unfused
PROT_CODES = 24  # protein tip codes: rows of the tip-vector table (plfx.h section 8)
CTX_LAZY_TABLES = 1  # PLFX_CTX_LAZY_TABLES
LOG_MINLIK = -22.18070977791824990137  # log(2^-32): one rescale's share of a log-likelihood (plf_lnl.hpp kLogMinLik)


class PlfxError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"plfx error {code}: {msg}")
        self.code = code


class Node(C.Structure):
    """plfx_node: one inner-node update (all device pointers)."""
    _fields_ = [("x1", C.c_void_p), ("x2", C.c_void_p), ("x3", C.c_void_p),
                ("left", C.c_void_p), ("right", C.c_void_p), ("scaler", C.c_void_p),
                ("scaler_sum", C.c_void_p)]


class PsrNode(C.Structure):
    """plfx_psr_node: one per-site-rate node (all device pointers)."""
    _fields_ = [("tip1", C.c_void_p), ("x1", C.c_void_p), ("tip2", C.c_void_p), ("x2", C.c_void_p),
                ("x3", C.c_void_p), ("left", C.c_void_p), ("right", C.c_void_p), ("scaler", C.c_void_p),
                ("scaler_sum", C.c_void_p)]


class PsrEdge(C.Structure):
    """plfx_psr_edge: one branch of a batched per-site-rate sum table (all device pointers)."""
    _fields_ = [("tip1", C.c_void_p), ("x1", C.c_void_p), ("x2", C.c_void_p), ("sumtab", C.c_void_p)]


class TravOp(C.Structure):
    _fields_ = [("parent", C.c_int32), ("child1", C.c_int32), ("child2", C.c_int32),
                ("pmat", C.c_int32)]


class _TB(C.Structure):
    _fields_ = [("alignment_sites", C.c_uint64), ("parallel_instances", C.c_uint32),
                ("window_size", C.c_uint32), ("layout", C.c_int32), ("aie_type", C.c_int32)]


_lib = None


def load():
    """Load libplfx.so.  torch is imported first (when present) so that the
    library binds to the same HIP runtime instance as torch's allocations."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  -- share torch's libamdhip64
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise PlfxError(ERR_UNSUPPORTED, f"{LIB_PATH} not built (run __graft_entry__.build())")
    L = C.CDLL(str(LIB_PATH))
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.plfx_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.plfx_ctx_create_ex.argtypes = [i32, C.c_uint, C.POINTER(vp)]
    L.plfx_ctx_destroy.argtypes = [vp]
    L.plfx_last_error.argtypes = [vp]
    L.plfx_last_error.restype = C.c_char_p
    L.plfx_ctx_stream.argtypes = [vp]
    L.plfx_ctx_stream.restype = vp
    L.plfx_ctx_device.argtypes = [vp]
    L.plfx_ctx_synchronize.argtypes = [vp]
    L.plfx_ctx_release_stream.argtypes = [vp, vp]
    L.plfx_ctx_set_streams.argtypes = [vp, i32]
    L.plfx_ctx_streams.argtypes = [vp]
    for s in ("f32", "f64"):
        getattr(L, f"plfx_plf_{s}").argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, C.POINTER(i32)]
        getattr(L, f"plfx_plf_dev_{s}").argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.plfx_instance_run.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, i32, i32, vp]
    L.plfx_instance_run_host.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, i32, i32]
    L.plfx_scaler_sum.argtypes = [vp, vp, vp, i64, vp, vp]
    tbp = C.POINTER(_TB)
    for name in ("alignments_per_instance", "instance_site_offset",
                 "instance_active_elements_left", "instance_active_elements_right"):
        f = getattr(L, f"plfx_tb_{name}")
        f.argtypes = [tbp, i32]
        f.restype = C.c_uint64
    for name in ("alignments_padding", "elements_per_instance", "instance_elements_left",
                 "instance_elements_right", "instance_elements_out", "num_windows_per_instance"):
        f = getattr(L, f"plfx_tb_{name}")
        f.argtypes = [tbp]
        f.restype = C.c_uint64
    L.plfx_pack_instance.argtypes = [tbp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.plfx_plf_dev_gen.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.plfx_plf_batch_dev.argtypes = [vp, i32, i32, C.POINTER(Node), i32, vp, i64, vp, vp]
    L.plfx_traverse.argtypes = [vp, i32, i32, C.POINTER(TravOp), i32, C.POINTER(vp), i32, vp, i32,
                                vp, i64, vp, C.POINTER(vp), vp, vp]
    L.plfx_root_lnl.argtypes = [vp, i32, i32, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp]
    dp = C.POINTER(C.c_double)
    L.plfx_model_eigen.argtypes = [i32, dp, dp, dp]
    L.plfx_gamma_rates.argtypes = [C.c_double, i32, i32, dp]
    L.plfx_model_ev.argtypes = [i32, i32, dp, dp]
    L.plfx_model_root_weights.argtypes = [i32, i32, dp, dp, dp]
    L.plfx_pmatrix.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, i64, vp, vp]
    L.plfx_model_tip_vectors.argtypes = [i32, i32, dp, dp]
    L.plfx_plf_tips_dev.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp,
                                    vp]
    L.plfx_plf_tips_dev_gen.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp,
                                        vp, vp, vp, vp]
    L.plfx_traverse_tips.argtypes = [vp, i32, i32, i32, C.POINTER(TravOp), i32, C.POINTER(vp),
                                     C.POINTER(vp), i32, vp, i32, vp, i64, vp, C.POINTER(vp), vp, vp,
                                     vp]
    u64p = C.POINTER(C.c_uint64)
    L.plfx_shard.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]
    L.plfx_gen_hostmem.argtypes = [i32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp]
    L.plfx_swemu_instance_run.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, i32, i32, i32]
    L.plfx_traverse_schedule.argtypes = [vp, C.POINTER(i32), i32]
    L.plfx_edge_sumtable.argtypes = [vp, i32, i32, vp, vp, vp, i64, vp, vp, vp]
    L.plfx_edge_derivatives.argtypes = [vp, i32, i32, vp, i64, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    dbl = C.c_double
    L.plfx_edge_optimize.argtypes = [vp, i32, i32, vp, i64, vp, vp, i32, vp, vp, dbl, dbl, dbl, i32,
                                     dp, dp, C.POINTER(i32), vp]
    L.plfx_edge_optimize_dev.argtypes = [vp, i32, i32, C.POINTER(vp), i32, i64, vp, vp, i32, vp, vp, vp, dbl, dbl,
                                         i32, vp, vp, vp, vp]
    # the per-site-rate entries (the arguments after ctx and dtype) and their _gen twins, which take states first
    pvp, top, dbl3 = C.POINTER(vp), C.POINTER(TravOp), [dbl, dbl, dbl]
    for name, args in (
            ("plfx_plf_psr_dev", [C.POINTER(PsrNode), i32, vp, i64, vp, i32, vp, vp, vp]),
            ("plfx_traverse_psr", [top, i32, pvp, pvp, i32, vp, i32, vp, i64, vp, i32, vp, pvp, vp, vp, vp]),
            ("plfx_root_lnl_psr", [vp, i64, vp, vp, vp, i32, vp, vp, vp]),
            ("plfx_edge_sumtable_psr", [vp, vp, vp, i64, vp, vp, vp]),
            ("plfx_edge_sumtable_psr_batch", [C.POINTER(PsrEdge), i32, i64, vp, vp]),
            ("plfx_edge_derivatives_psr", [vp, i64, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]),
            ("plfx_edge_optimize_psr", [vp, i64, vp, vp, i32, vp, vp] + dbl3 + [i32, dp, dp, C.POINTER(i32), vp]),
            ("plfx_edge_optimize_psr_dev", [pvp, i32, i64, vp, vp, i32, vp, vp, vp, dbl, dbl, i32, vp, vp, vp, vp])):
        getattr(L, name).argtypes = [vp, i32] + args
        getattr(L, name + "_gen").argtypes = [vp, i32, i32] + args
    # the rate scan (section 12) and its _gen twins (12b): states after dtype
    for name, head, args in (
            ("plfx_site_lnl_psr", [vp, i32], [vp, i64, vp, vp, i32, i64, vp, vp]),
            ("plfx_psr_rate_scan", [vp, i32], [top, i32, pvp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, i64, vp,
                                               C.c_size_t, vp, vp, vp, vp, vp]),
            ("plfx_psr_rate_scan_workspace", [i32], [i32, i32, i32, i64, i32, C.POINTER(C.c_size_t)])):
        getattr(L, name).argtypes = head + args
        getattr(L, name + "_gen").argtypes = head + [i32] + args
    # the PROTCAT FMA entries (section 11d): their _gen bases with flags after states
    for name in ("plfx_plf_psr_dev", "plfx_traverse_psr", "plfx_psr_rate_scan"):
        base = getattr(L, name + "_gen").argtypes
        getattr(L, name + "_ex").argtypes = base[:3] + [i32] + base[3:]
    # all-branch derivatives (section 13)
    L.plfx_branch_sumtables_psr_workspace.argtypes = [i32, i32, i32, i64, C.POINTER(C.c_size_t)]
    L.plfx_branch_sumtables_psr.argtypes = [vp, i32, i32, i32, top, i32, pvp, pvp, i32, vp, i32, vp, vp, i64, vp, i32,
                                            vp, vp, vp, vp, C.c_size_t, pvp, vp, vp]
    L.plfx_branch_pair_sites_per_lane.argtypes = [i32]
    L.plfx_psr_categorize.argtypes = [dp, i32, vp, vp, i64, i32, vp, dp, C.POINTER(i32), dp]
    L.plfx_psr_site_order.argtypes = [vp, i64, i32, vp]
    _lib = L
    return L


class Context:
    """A libplfx context bound to one HIP device (replaces acap_info,
    app/src/include.h:28-147).  lazy_tables=True (PLFX_CTX_LAZY_TABLES, for
    DNA-only users): the protein tip/tip tables are allocated on a stream's
    first tip/tip call instead of with the context (~95 MB)."""

    def __init__(self, device: int = 0, lazy_tables: bool = False):
        self._L = load()
        h = C.c_void_p()
        rc = self._L.plfx_ctx_create_ex(int(device), CTX_LAZY_TABLES if lazy_tables else 0, C.byref(h))
        if rc != OK:
            raise PlfxError(rc, f"plfx_ctx_create(device={device}) failed "
                                "(no gfx950 device visible?)")
        self.h = h
        self.device = device
        self._used = {}  # torch streams this context ran on: released at close()

    def _sh(self, stream):
        """The hipStream_t of `stream` (None: torch's current stream on the
        context's device), remembering torch streams so that close() can
        release their workspaces (plfx_ctx_release_stream) and destroy stays
        off the device-wide wait.  Raw integer handles are not remembered (the
        stream may be destroyed before the context): release those yourself."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device)
        if not isinstance(stream, int):
            self._used[stream.cuda_stream] = stream
        return _stream_handle(stream, self.device)

    def close(self):
        if getattr(self, "h", None):
            for st in list(getattr(self, "_used", {}).values()):
                try:  # refused (and left to destroy) while the stream is being captured
                    self._L.plfx_ctx_release_stream(self.h, C.c_void_p(st.cuda_stream))
                except Exception:
                    pass
            self._used = {}
            self._L.plfx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def stream(self):
        return self._L.plfx_ctx_stream(self.h)

    def synchronize(self):
        self._check(self._L.plfx_ctx_synchronize(self.h))

    @property
    def streams(self):
        """One-node calls kept in flight (plfx_ctx_streams)."""
        return self._L.plfx_ctx_streams(self.h)

    def set_streams(self, streams):
        """Tell the context that `streams` one-node calls run at once, each on
        its own stream (plfx_ctx_set_streams: the dense DNA node and f64
        protein FMA kernels then launch the resident blocks / streams)."""
        self._check(self._L.plfx_ctx_set_streams(self.h, int(streams)))

    def release_stream(self, stream):
        """Wait for `stream` and return its scaler-sum workspace to the pool
        (plfx_ctx_release_stream)."""
        h = _stream_handle(stream, self.device)
        self._check(self._L.plfx_ctx_release_stream(self.h, h))
        self._used.pop(h.value, None)

    def _check(self, rc):
        if rc != OK:
            raise PlfxError(rc, self._L.plfx_last_error(self.h).decode(errors="replace"))

    def _call(self, name, dt, states, psr, gen, *args, flags=None):
        """Call the C entry `name` on tensors of dtype dt.  A Gamma entry takes
        the state count after the dtype; a per-site-rate entry (psr) is
        `name`, or with gen its _gen twin, which alone takes the state count;
        with flags (section 11d) the _gen twin's _ex form, flags after states."""
        import torch

        if flags is not None:
            fn = getattr(self._L, name + "_ex")
            self._check(fn(self.h, F32 if dt == torch.float32 else F64, states, int(flags), *args))
            return
        fn = getattr(self._L, name + ("_gen" if psr and gen else ""))
        self._check(fn(self.h, F32 if dt == torch.float32 else F64, *((states,) if gen or not psr else ()), *args))

    # -- (1) plf() drop-in on host arrays ----------------------------------
    def plf(self, x1_start, x2_start, x3_start, EV, n, left, right, wgt=None):
        """plf(x1, x2, x3, EV, n, left, right, wgt) -> scalerIncrement.

        numpy float32 or float64 arrays, x3_start written in place."""
        dt = np.asarray(x1_start).dtype
        if dt not in (np.float32, np.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        arrs = [x1_start, x2_start, x3_start, EV, left, right]
        for a in arrs:
            if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
                raise PlfxError(ERR_INVALID, "arrays must be C-contiguous numpy arrays of one dtype")
        n = int(n)
        if x1_start.size < 16 * n or x2_start.size < 16 * n or x3_start.size < 16 * n:
            raise PlfxError(ERR_INVALID, "CLV arrays shorter than 16*n")
        if EV.size < 16 or left.size < 64 or right.size < 64:
            raise PlfxError(ERR_INVALID, "EV needs 16, left/right 64 values")
        w = None
        if wgt is not None:
            w = np.ascontiguousarray(wgt, dtype=np.int32)
            if w.size < n:
                raise PlfxError(ERR_INVALID, "wgt shorter than n")
        inc = C.c_int(0)
        fn = self._L.plfx_plf_f32 if dt == np.float32 else self._L.plfx_plf_f64
        p = _nptr
        self._check(fn(self.h, p(x1_start), p(x2_start), p(x3_start), p(EV), n, p(left), p(right),
                       p(w), C.byref(inc)))
        return inc.value

    # -- (2) device-resident hot path ---------------------------------------
    def plf_dev(self, x1, x2, x3, EV, left, right, wgt=None, scaler=None, scaler_sum=None,
                n=None, stream=None):
        """Fused PLF on torch device tensors (float32/float64, contiguous).

        Asynchronous on `stream` (a torch.cuda.Stream, a raw hipStream_t int,
        or None = torch's current stream)."""
        import torch

        dt = x1.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        n = x1.numel() // 16 if n is None else int(n)
        for k, t, m in (("x1", x1, 16 * n), ("x2", x2, 16 * n), ("x3", x3, 16 * n), ("EV", EV, 16),
                        ("left", left, 64), ("right", right, 64)):
            _tensor(t, k, dt, m)
        _check_aux(n, wgt, scaler, scaler_sum)
        fn = self._L.plfx_plf_dev_f32 if dt == torch.float32 else self._L.plfx_plf_dev_f64
        p = _ptr
        self._check(fn(self.h, p(x1), p(x2), p(x3), p(EV), n, p(left), p(right), p(wgt),
                       p(scaler), p(scaler_sum), self._sh(stream)))

    def bind_plf_dev(self, x1, x2, x3, EV, left, right, wgt=None, scaler=None, scaler_sum=None,
                     n=None):
        """Validate once and return a launcher ``run(stream=None)`` that issues
        the same fused PLF call with no per-call Python checks (for launch-rate
        bound loops: a 1M-site f64 call is ~67 us of GPU time).  The launcher
        holds references to the tensors, so their memory stays allocated while
        it lives (a graph captured through it, too, needs it alive); the
        tensors must keep their shape and device."""
        import torch

        self.plf_dev(x1, x2, x3, EV, left, right, wgt, scaler, scaler_sum, n=n,
                     stream=torch.cuda.current_stream(x1.device).cuda_stream)  # validates
        n = x1.numel() // 16 if n is None else int(n)
        fn = self._L.plfx_plf_dev_f32 if x1.dtype == torch.float32 else self._L.plfx_plf_dev_f64
        p = _ptr
        args = (self.h, p(x1), p(x2), p(x3), p(EV), C.c_int64(n), p(left), p(right), p(wgt),
                p(scaler), p(scaler_sum))
        check = self._check
        held = (x1, x2, x3, EV, left, right, wgt, scaler, scaler_sum)  # raw pointers in args

        def run(stream=None):
            if self.h is None:  # args carry the handle: a closed context's would dangle
                raise PlfxError(ERR_INVALID, "launcher used after its context was closed")
            check(fn(*args, self._sh(stream)))

        run.tensors = held
        return run

    # -- (3) instance-buffer contract --------------------------------------
    def instance_run(self, in_left, in_right, out_clv, out_scaler, alignment_sites, window_size,
                     layout, stream=None):
        import torch

        dt = in_left.dtype
        if dt not in (torch.float32, torch.float64) or in_right.dtype != dt or out_clv.dtype != dt:
            raise PlfxError(ERR_INVALID, "instance buffers must share a float dtype")
        hdr_r = 80 if layout == LAYOUT_COMBINED else 64
        n = int(alignment_sites)
        if in_left.numel() < 80 + 16 * n or in_right.numel() < hdr_r + 16 * n or \
                out_clv.numel() < 16 * n:
            raise PlfxError(ERR_INVALID, "instance buffers too small for alignment_sites")
        if out_scaler is not None and (out_scaler.dtype != torch.uint8 or out_scaler.numel() < n):
            raise PlfxError(ERR_INVALID, "out_scaler must be uint8 with >= alignment_sites bytes")
        p = _ptr
        self._check(self._L.plfx_instance_run(self.h, p(in_left), p(in_right), p(out_clv),
                                              p(out_scaler), n, int(window_size), int(layout),
                                              F32 if dt == torch.float32 else F64,
                                              self._sh(stream)))

    def instance_run_host(self, in_left, in_right, out_clv, out_scaler, alignment_sites,
                          window_size, layout):
        """instance_run on numpy host buffers, synchronous (bo.write -> run ->
        bo.read, host_mem.cpp:293-318)."""
        import numpy as np

        dt = in_left.dtype
        if dt not in (np.float32, np.float64) or in_right.dtype != dt or out_clv.dtype != dt:
            raise PlfxError(ERR_INVALID, "instance buffers must share a float dtype")
        hdr_r = 80 if layout == LAYOUT_COMBINED else 64
        n = int(alignment_sites)
        if in_left.size < 80 + 16 * n or in_right.size < hdr_r + 16 * n or out_clv.size < 16 * n:
            raise PlfxError(ERR_INVALID, "instance buffers too small for alignment_sites")
        if out_scaler is not None and (out_scaler.dtype != np.uint8 or out_scaler.size < n):
            raise PlfxError(ERR_INVALID, "out_scaler must be uint8 with >= alignment_sites bytes")
        for a in (in_left, in_right, out_clv, out_scaler):
            if a is not None and not a.flags.c_contiguous:
                raise PlfxError(ERR_INVALID, "instance buffers must be C-contiguous")
        p = _nptr
        self._check(self._L.plfx_instance_run_host(self.h, p(in_left), p(in_right), p(out_clv),
                                                   p(out_scaler), n, int(window_size), int(layout),
                                                   F32 if dt == np.float32 else F64))

    def plf_dev_gen(self, x1, x2, x3, EV, left, right, states, wgt=None, scaler=None,
                    scaler_sum=None, n=None, fma=False, stream=None, valu=False):
        """Any built state count (4 DNA, 20 protein), 4 Gamma categories, on
        torch device tensors: x[site][cat][state], P [cat][k][l], EV [k][l].
        fma: PLFX_FMA; valu (with fma, protein f64): the same fused chains on
        the VALU instead of the matrix cores, P and EV as wave-uniform scalar
        operands, LDS holding only the staged child tile (PLFX_VALU;
        bit-identical)."""
        import torch

        V, S2 = 4 * states, states * states
        dt = x1.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        n = x1.numel() // V if n is None else int(n)
        for k, t, m in (("x1", x1, V * n), ("x2", x2, V * n), ("x3", x3, V * n), ("EV", EV, S2),
                        ("left", left, 4 * S2), ("right", right, 4 * S2)):
            _tensor(t, k, dt, m)
        _check_aux(n, wgt, scaler, scaler_sum)
        p = _ptr
        self._check(self._L.plfx_plf_dev_gen(self.h, F32 if dt == torch.float32 else F64, int(states),
                                             (FMA if fma else EXACT) | (VALU if valu else 0),
                                             p(x1), p(x2), p(x3), p(EV), n,
                                             p(left), p(right), p(wgt), p(scaler), p(scaler_sum),
                                             self._sh(stream)))

    # -- (6) batched nodes / traversal ---------------------------------------
    def plf_batch_dev(self, nodes, EV, n, wgt=None, stream=None, states=4):
        """nodes: sequence of dicts with torch tensors x1, x2, x3, left, right and
        optional scaler (uint8[n]), scaler_sum (int64[1]); all one float dtype,
        all sharing EV, n (sites) and wgt."""
        import torch

        dt = EV.dtype
        V, M = 4 * states, 4 * states * states
        arr = (Node * len(nodes))()
        for i, nd in enumerate(nodes):
            for k in ("x1", "x2", "x3"):
                _tensor(nd[k], f"node {i}: {k}", dt, V * n)
            for k in ("left", "right"):
                _tensor(nd[k], f"node {i}: {k}", dt, M)
            try:
                _check_aux(n, None, nd.get("scaler"), nd.get("scaler_sum"))
            except PlfxError as e:
                raise PlfxError(ERR_INVALID, f"node {i}: {e}") from None
            arr[i] = _node(nd)
        _check_aux(n, wgt, None, None)
        _tensor(EV, "EV", dt, states * states)
        self._check(self._L.plfx_plf_batch_dev(self.h, F32 if dt == torch.float32 else F64, states, arr,
                                               len(nodes), _ptr(EV), int(n), _ptr(wgt), self._sh(stream)))

    def bind_plf_batch_dev(self, nodes, EV, n, wgt=None, states=4):
        """Validate once (as plf_batch_dev) and return a launcher
        ``run(stream=None)`` issuing the same batched call with a prebuilt
        node array (graph capture / launch-rate bound loops).  The launcher
        holds references to every node's tensors, EV and wgt, so their memory
        stays allocated while it lives."""
        import torch

        if not nodes:
            return lambda stream=None: None
        self.plf_batch_dev(nodes, EV, n, wgt, stream=torch.cuda.current_stream(self.device).cuda_stream,
                           states=states)  # validates
        arr = (Node * len(nodes))(*[_node(nd) for nd in nodes])
        fn, h, check = self._L.plfx_plf_batch_dev, self.h, self._check
        args = (F32 if EV.dtype == torch.float32 else F64, states, arr, len(nodes), _ptr(EV), int(n), _ptr(wgt))

        ctx = self

        def run(stream=None):
            if ctx.h is None:  # h would dangle
                raise PlfxError(ERR_INVALID, "launcher used after its context was closed")
            check(fn(h, *args, ctx._sh(stream)))

        run.tensors = ([dict(nd) for nd in nodes], EV, wgt)  # raw pointers in arr / args
        return run

    def traverse(self, ops, clv, pmats, EV, n, wgt=None, scalers=None, scaler_sums=None,
                 stream=None, tips=None, tipvec=None, states=4, fma=False):
        """Run a post-order traversal descriptor.  ops: (nops, 4) int array of
        [parent, child1, child2, pmat]; clv: list of torch CLV tensors (slots;
        None where the slot is a tip); pmats: tensor of 2*npmat matrices (64
        values each for DNA); tips: optional list (per slot) of uint8 code
        tensors or None (plfx.h section 8: DNA state bits, protein code
        indices); tipvec: optional device table of tip vectors (16 x 4 DNA,
        PROT_CODES x 20 protein; dtype of the CLVs); states 4 or 20, fma:
        PLFX_FMA for protein nodes."""
        import torch

        dt = EV.dtype
        S2 = states * states
        top, nops, slots, tp, nslots, npmats, sc = self._traverse_args(
            ops, clv, pmats, EV, n, wgt, scalers, scaler_sums, tips, 4 * states, 4 * S2, S2)
        self._check(self._L.plfx_traverse_tips(
            self.h, F32 if dt == torch.float32 else F64, states, FMA if fma else EXACT, top, nops,
            slots, tp, nslots, _ptr(pmats), npmats, _ptr(EV), int(n), _ptr(wgt), sc, _ptr(scaler_sums),
            self._tipvec(tipvec, dt, states), self._sh(stream)))

    @staticmethod
    def _traverse_args(ops, clv, pmats, EV, n, wgt, scalers, scaler_sums, tips, V, M, ev):
        """What traverse() and traverse_psr() share: the checks of the call's
        tensors -- V values per CLV site, M per matrix, ev in EV, all of EV's
        dtype -- and the ctypes arrays.  Returns (ops, nops, slots, tips,
        nslots, npmats, scalers)."""
        import torch

        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 4)
        nops, nslots, dt = ops.shape[0], len(clv), EV.dtype
        if tips is not None and len(tips) != nslots:
            raise PlfxError(ERR_INVALID, "tips must have one entry per slot")
        for s_, t in enumerate(clv):
            if tips is not None and tips[s_] is not None:
                _tensor(tips[s_], f"tip slot {s_}", torch.uint8, n)
            else:
                _tensor(t, f"CLV slot {s_}", dt, V * n)
        _tensor(pmats, "pmats", dt, 0)
        if pmats.numel() % (2 * M):
            raise PlfxError(ERR_INVALID, f"pmats must hold whole (left, right) pairs of {M} values")
        _tensor(scaler_sums, "scaler_sums", torch.int64, nops, contiguous=False, optional=True)
        if scalers is not None:
            if len(scalers) > nops:
                raise PlfxError(ERR_INVALID, "more scaler tensors than ops")
            scalers = list(scalers) + [None] * (nops - len(scalers))
            for j, t in enumerate(scalers):
                _tensor(t, f"scaler of op {j}", torch.uint8, n, optional=True)
        _check_aux(n, wgt, None, None)
        _tensor(EV, "EV", dt, ev)
        # at least one element: with no ops the library follows neither array
        top = (TravOp * max(1, nops))(*[TravOp(*map(int, r)) for r in ops])
        slots = (C.c_void_p * nslots)(*map(_ptr, clv))
        tp = None if tips is None else (C.c_void_p * nslots)(*map(_ptr, tips))
        sc = None if scalers is None else (C.c_void_p * max(1, nops))(*map(_ptr, scalers))
        return top, nops, slots, tp, nslots, pmats.numel() // (2 * M), sc

    @staticmethod
    def _tipvec(tipvec, dt, states=4):
        if tipvec is None:
            return C.c_void_p(None)
        rows, width = (16, 4) if states == 4 else (PROT_CODES, 20)
        if tipvec.dtype != dt or tipvec.numel() < rows * width or not tipvec.is_contiguous():
            raise PlfxError(ERR_INVALID, f"tipvec must be a contiguous device table of "
                                         f"{rows} x {width} values")
        return C.c_void_p(tipvec.data_ptr())

    def plf_tips_dev(self, x3, EV, n, left, right, x1=None, x2=None, tip1=None, tip2=None,
                     wgt=None, scaler=None, scaler_sum=None, tipvec=None, stream=None, states=4,
                     fma=False):
        """One inner node with tip children (plfx.h section 8): for each child
        pass exactly one of the dense CLV (x1/x2) or the uint8 codes
        (tip1/tip2).  states 4 (DNA state bits) or 20 (protein code indices,
        PROT_CODES rows); fma: PLFX_FMA (protein)."""
        import torch

        dt = EV.dtype
        S2 = states * states
        for k, t in (("x3", x3), ("x1", x1), ("x2", x2)):
            _tensor(t, k, dt, 4 * states * n, optional=True)
        for k, t in (("tip1", tip1), ("tip2", tip2)):
            _tensor(t, k, torch.uint8, n, optional=True)
        for k, t, m in (("EV", EV, S2), ("left", left, 4 * S2), ("right", right, 4 * S2)):
            _tensor(t, k, dt, m, contiguous=False)
        _check_aux(n, wgt, scaler, scaler_sum)
        p = _ptr
        self._check(self._L.plfx_plf_tips_dev_gen(
            self.h, F32 if dt == torch.float32 else F64, states, FMA if fma else EXACT, p(tip1),
            p(x1), p(tip2), p(x2), p(x3), p(EV), int(n), p(left), p(right), p(wgt), p(scaler),
            p(scaler_sum), self._tipvec(tipvec, dt, states), self._sh(stream)))

    def last_schedule(self):
        """The schedule the last traverse() on this context chose
        (plfx_traverse_schedule): dict over SCHED_KEYS."""
        c = (C.c_int * len(SCHED_KEYS))()
        m = self._L.plfx_traverse_schedule(self.h, c, len(SCHED_KEYS))
        return {k: int(c[i]) for i, k in enumerate(SCHED_KEYS[:m])}

    # -- (9) P matrices from branch lengths --------------------------------
    def pmatrix(self, eigen, rates, blen, out, states=4, convention=PMAT_STATE, stream=None):
        """out[b][c][k][l] from a device eigensystem (float64, S+2S^2), device
        category rates (float64) and branch lengths (float64); plfx.h (9)."""
        import torch

        S = states
        _tensor(eigen, "eigen", torch.float64, S + 2 * S * S)
        _tensor(rates, "rates", torch.float64, 0)
        _tensor(blen, "blen", torch.float64, 0)
        ncat, nb = rates.numel(), blen.numel()
        _tensor(out, "out", (torch.float32, torch.float64), nb * ncat * S * S)
        self._check(self._L.plfx_pmatrix(
            self.h, F32 if out.dtype == torch.float32 else F64, S, convention, _ptr(eigen), _ptr(rates), ncat,
            _ptr(blen), nb, _ptr(out), self._sh(stream)))

    # -- (7) root log-likelihood --------------------------------------------
    def root_lnl(self, x, n, out, catw=None, freq=None, wgt=None, scaler_sums=None,
                 site_lnl=None, states=4, stream=None):
        """Root lnL into `out` (float64 device tensor, 1 element); see plfx.h (7)."""
        self._root_lnl(False, False, states, x, n, out, catw, freq, wgt, scaler_sums, site_lnl, stream)

    def _root_lnl(self, psr, gen, states, x, n, out, catw, freq, wgt, scaler_sums, site_lnl, stream):
        """root_lnl (4 * states values per site) and root_lnl_psr[_gen] (states)."""
        import torch

        if psr:
            states = self._psr_states(gen, states)
        _tensor(out, "out", torch.float64, 1, contiguous=False)
        _tensor(x, "x", (torch.float32, torch.float64), (1 if psr else 4) * states * n)
        for k, t, m in (("catw", catw, 4), ("freq", freq, states), ("site_lnl", site_lnl, n)):
            _tensor(t, k, torch.float64, m, optional=True)
        _check_aux(n, wgt, None, None)
        _tensor(scaler_sums, "scaler_sums", torch.int64, 0, optional=True)
        nsums = 0 if scaler_sums is None else scaler_sums.numel()
        self._call("plfx_root_lnl_psr" if psr else "plfx_root_lnl", x.dtype, states, psr, gen, _ptr(x), int(n),
                   *(() if psr else (_ptr(catw),)), _ptr(freq), _ptr(wgt), _ptr(scaler_sums), nsums, _ptr(out),
                   _ptr(site_lnl), self._sh(stream))

    # -- (10) one branch between two fixed CLVs -----------------------------
    def edge_sumtable(self, x2, sumtab, n, x1=None, tip1=None, tipvec=None, states=4, stream=None):
        """sumtab = x1 * x2 elementwise (plfx.h (10)); side 1 is the dense CLV
        x1 or the uint8 codes tip1 with the eigen-convention table tipvec
        (16 x 4 DNA, PROT_CODES x 20 protein).  CLVs in the eigen convention."""
        self._edge_sumtable(False, False, states, x2, sumtab, n, x1, tip1, tipvec, stream)

    def _edge_sumtable(self, psr, gen, states, x2, sumtab, n, x1, tip1, tipvec, stream):
        """edge_sumtable (4 * states values per site) and edge_sumtable_psr[_gen] (states)."""
        import torch

        if psr:
            states = self._psr_states(gen, states)
        dt = sumtab.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        for k, t in (("x1", x1), ("x2", x2), ("sumtab", sumtab)):
            _tensor(t, k, dt, (1 if psr else 4) * states * n, optional=True)
        _tensor(tip1, "tip1", torch.uint8, n, optional=True)
        self._call("plfx_edge_sumtable_psr" if psr else "plfx_edge_sumtable", dt, int(states), psr, gen, _ptr(tip1),
                   _ptr(x1), _ptr(x2), int(n), self._tipvec(tipvec, dt, states), _ptr(sumtab), self._sh(stream))

    def _edge_args(self, name, psr, gen, states, sumtab, n, eigen, rates, cat, wgt):
        """What the edge calls share, checked: the Gamma ones (4 * states values
        per site, cat = catw) and the per-site-rate ones (psr: states values,
        cat = rate_cat).  name: the C entry, with %s where its PSR form has
        _psr.  Returns (call, tail): call(table(s), *tail, ...) is the call."""
        import torch

        if psr:
            states = self._psr_states(gen, states)
        _tensor(sumtab, "sumtab", (torch.float32, torch.float64), (1 if psr else 4) * states * n)
        ncat = rates.numel()
        _tensor(eigen, "eigen", torch.float64, states, optional=True)
        _tensor(rates, "rates", torch.float64, 1)
        if psr:
            _tensor(cat, "rate_cat", torch.uint8, n)
        else:
            _tensor(cat, "catw", torch.float64, ncat, optional=True)
        _check_aux(n, wgt, None, None)
        call = functools.partial(self._call, name % ("_psr" if psr else ""), sumtab.dtype, int(states), psr, gen)
        return call, (int(n), _ptr(eigen), _ptr(rates), ncat, _ptr(cat), _ptr(wgt))

    def edge_derivatives(self, sumtab, n, eigen, rates, t, out, catw=None, wgt=None, scaler_sums=None,
                         site_lnl=None, states=4, stream=None):
        """out (float64 device tensor, 3 elements) = lnL, d lnL/dt, d2 lnL/dt2 of
        the branch whose sum table is `sumtab`, at the branch length in the
        device double `t`; see plfx.h (10).  eigen, rates: the device arrays
        pmatrix() takes."""
        self._edge_derivatives(False, False, states, sumtab, n, eigen, rates, catw, wgt, t, out, scaler_sums,
                               site_lnl, stream)

    def _edge_derivatives(self, psr, gen, states, sumtab, n, eigen, rates, cat, wgt, t, out, scaler_sums, site_lnl,
                          stream):
        """edge_derivatives and edge_derivatives_psr[_gen] after their _edge_args."""
        import torch

        call, tail = self._edge_args("plfx_edge_derivatives%s", psr, gen, states, sumtab, n, eigen, rates, cat, wgt)
        for k, x, m in (("t", t, 1), ("out", out, 3), ("site_lnl", site_lnl, n)):
            _tensor(x, k, torch.float64, m, optional=True)
        if t is None or out is None:
            raise PlfxError(ERR_INVALID, "t and out are required")
        _tensor(scaler_sums, "scaler_sums", torch.int64, 0, optional=True)
        nsums = 0 if scaler_sums is None else scaler_sums.numel()
        call(_ptr(sumtab), *tail, _ptr(t), _ptr(scaler_sums), nsums, _ptr(out), _ptr(site_lnl), self._sh(stream))

    def optimize_branch(self, sumtab, n, eigen, rates, t0, tmin=1e-8, tmax=10.0, max_evals=64,
                        catw=None, wgt=None, states=4, stream=None):
        """The branch length in [tmin, tmax] maximising the edge lnL, by the
        bracketed Newton iteration of plfx_edge_optimize from t0 (host-
        synchronous).  Returns (t, lnL, d1, d2, evals), lnL without a scaling
        correction."""
        return self._optimize_branch(False, False, states, sumtab, n, eigen, rates, catw, wgt, t0, tmin, tmax,
                                     max_evals, stream)

    def _optimize_branch(self, psr, gen, states, sumtab, n, eigen, rates, cat, wgt, t0, tmin, tmax, max_evals, stream):
        """optimize_branch and optimize_branch_psr[_gen] after their _edge_args."""
        call, tail = self._edge_args("plfx_edge_optimize%s", psr, gen, states, sumtab, n, eigen, rates, cat, wgt)
        t, out, ev = C.c_double(0.0), (C.c_double * 3)(), C.c_int(0)
        call(_ptr(sumtab), *tail, float(t0), float(tmin), float(tmax), int(max_evals), C.byref(t), out, C.byref(ev),
             self._sh(stream))
        return t.value, out[0], out[1], out[2], ev.value

    def optimize_branches(self, sumtabs, n, eigen, rates, t0, t_opt, tmin=1e-8, tmax=10.0, max_evals=64,
                          out3=None, evals=None, catw=None, wgt=None, states=4, stream=None):
        """optimize_branch for the independent branches whose sum tables are the
        device tensors in `sumtabs`, with the loop on the device
        (plfx_edge_optimize_dev): asynchronous, no synchronisation, capture-
        safe.  t0, t_opt: float64 device tensors of len(sumtabs) (t0 is read
        on the device: another call's t_opt may be passed); out3 (3 per
        branch, float64) and evals (int32) are optional device tensors."""
        self._optimize_branches(False, False, states, sumtabs, n, eigen, rates, catw, wgt, t0, t_opt, tmin, tmax,
                                max_evals, out3, evals, stream)

    def _optimize_branches(self, psr, gen, states, sumtabs, n, eigen, rates, cat, wgt, t0, t_opt, tmin, tmax,
                           max_evals, out3, evals, stream):
        """optimize_branches and optimize_branches_psr[_gen] after their _edge_args."""
        import torch

        m = len(sumtabs)
        if m < 1:
            raise PlfxError(ERR_INVALID, "sumtabs must hold at least one sum table")
        for st in sumtabs:
            if st.dtype != sumtabs[0].dtype:
                raise PlfxError(ERR_INVALID, "the sum tables must share one dtype")
            call, tail = self._edge_args("plfx_edge_optimize%s_dev", psr, gen, states, st, n, eigen, rates, cat, wgt)
        for k, x, cnt, dt in (("t0", t0, m, torch.float64), ("t_opt", t_opt, m, torch.float64),
                              ("out3", out3, 3 * m, torch.float64), ("evals", evals, m, torch.int32)):
            _tensor(x, k, dt, cnt, optional=True)
        if t0 is None or t_opt is None:
            raise PlfxError(ERR_INVALID, "t0 and t_opt are required")
        tabs = (C.c_void_p * m)(*[st.data_ptr() for st in sumtabs])
        call(tabs, m, *tail, _ptr(t0), float(tmin), float(tmax), int(max_evals), _ptr(t_opt), _ptr(out3), _ptr(evals),
             self._sh(stream))

    # -- (11) per-site rate categories; (11b, 11c) the _gen twins, with a state count: one body each, taking gen --
    @staticmethod
    def _psr_states(gen, states):
        """The state counts built: 4 alone through the section-11 entries, 4 and 20 through their _gen twins."""
        if states not in ((4, 20) if gen else (4,)):
            raise PlfxError(ERR_UNSUPPORTED,
                            f"per-site rate categories: states={states} not built ({'4, 20' if gen else '4'})")
        return int(states)

    def plf_psr(self, nodes, EV, n, rate_cat, ncat, wgt=None, tipvec=None, states=4, stream=None):
        """Per-site-rate node updates (plfx.h section 11).  nodes: one dict or
        a list of dicts with x3, left, right and, per child, exactly one of
        x1 / tip1 and one of x2 / tip2 (dense CLVs of 4*n values, or uint8
        codes), plus optional scaler, scaler_sum.  rate_cat: uint8 device
        tensor, one category per site (values >= ncat count as ncat - 1);
        left / right hold ncat * 16 values."""
        self._plf_psr(False, states, nodes, EV, n, rate_cat, ncat, wgt, tipvec, stream)

    def plf_psr_gen(self, states, nodes, EV, n, rate_cat, ncat, wgt=None, tipvec=None, stream=None, fma=False):
        """plf_psr() with a state count (plfx.h section 11b): states 4 is
        plf_psr() itself, states 20 the protein node -- CLVs of 20*n values,
        left / right of ncat * 400, EV of 400, uint8 protein codes (PROT_CODES
        rows of 20 in tipvec, None = the default table).  Fast when the sites
        are sorted by category: see psr_site_order().  fma: PLFX_FMA through
        plfx_plf_psr_dev_ex (section 11d) -- with 20 states every multiply-add
        fused on the f64 matrix cores (float64 only); 4 states stay exact."""
        self._plf_psr(True, states, nodes, EV, n, rate_cat, ncat, wgt, tipvec, stream, FMA if fma else None)

    def _plf_psr(self, gen, states, nodes, EV, n, rate_cat, ncat, wgt, tipvec, stream, flags=None):
        import torch

        S = self._psr_states(gen, states)
        if isinstance(nodes, dict):
            nodes = [nodes]
        n, ncat = int(n), int(ncat)
        dt = EV.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        _tensor(EV, "EV", dt, S * S, contiguous=False)
        _tensor(rate_cat, "rate_cat", torch.uint8, n)
        _check_aux(n, wgt, None, None)
        arr = (PsrNode * max(1, len(nodes)))()
        for i, nd in enumerate(nodes):
            for k in ("x1", "x2", "x3"):
                _tensor(nd.get(k), k, dt, S * n, optional=True)
            for k in ("tip1", "tip2"):
                _tensor(nd.get(k), k, torch.uint8, n, optional=True)
            for k in ("left", "right"):
                _tensor(nd.get(k), k, dt, S * S * max(ncat, 0), optional=True)
            _check_aux(n, None, nd.get("scaler"), nd.get("scaler_sum"))
            arr[i] = PsrNode(*(_ptr(nd.get(k)) for k in ("tip1", "x1", "tip2", "x2", "x3", "left", "right",
                                                          "scaler", "scaler_sum")))
        self._call("plfx_plf_psr_dev", dt, S, True, gen, arr, len(nodes), _ptr(EV), n, _ptr(rate_cat), ncat,
                   _ptr(wgt), self._tipvec(tipvec, dt, S), self._sh(stream), flags=flags)

    def traverse_psr(self, ops, clv, pmats, EV, n, rate_cat, ncat, wgt=None, scalers=None, scaler_sums=None,
                     stream=None, tips=None, tipvec=None, states=4):
        """A post-order traversal under per-site rate categories (plfx.h
        section 11, plfx_traverse_psr).  ops, clv, tips, scalers, scaler_sums
        as traverse(); a CLV slot holds 4*n values; pmats holds whole (left,
        right) pairs of ncat * 16 values each, as pmatrix() writes them for
        2*npmats branches and ncat rates; rate_cat, ncat, tipvec as plf_psr().
        Level pairs are fused only in a context created with PLFX_FUSE >= 1
        in the environment.  last_schedule() reports the call: triples,
        unfused, launches."""
        self._traverse_psr(False, states, ops, clv, pmats, EV, n, rate_cat, ncat, wgt, scalers, scaler_sums, stream,
                           tips, tipvec)

    def traverse_psr_gen(self, states, ops, clv, pmats, EV, n, rate_cat, ncat, wgt=None, scalers=None,
                         scaler_sums=None, stream=None, tips=None, tipvec=None, fma=False):
        """traverse_psr() with a state count (plfx.h section 11b).  With
        states 20 a CLV slot holds 20*n values, pmats whole (left, right) pairs
        of ncat * 400 values each, and no level pair is fused whatever
        PLFX_FUSE says: last_schedule() reports triples 0, unfused = the ops.
        fma: PLFX_FMA through plfx_traverse_psr_ex, as plf_psr_gen()."""
        self._traverse_psr(True, states, ops, clv, pmats, EV, n, rate_cat, ncat, wgt, scalers, scaler_sums, stream,
                           tips, tipvec, FMA if fma else None)

    def _traverse_psr(self, gen, states, ops, clv, pmats, EV, n, rate_cat, ncat, wgt, scalers, scaler_sums, stream,
                      tips, tipvec, flags=None):
        import torch

        S = self._psr_states(gen, states)
        n, ncat = int(n), int(ncat)
        dt = EV.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        top, nops, slots, tp, nslots, npmats, sc = self._traverse_args(
            ops, clv, pmats, EV, n, wgt, scalers, scaler_sums, tips, S, S * S * max(ncat, 1), S * S)
        _tensor(rate_cat, "rate_cat", torch.uint8, n)
        self._call("plfx_traverse_psr", dt, S, True, gen, top, nops, slots, tp, nslots, _ptr(pmats), npmats, _ptr(EV),
                   n, _ptr(rate_cat), ncat, _ptr(wgt), sc, _ptr(scaler_sums), self._tipvec(tipvec, dt, S),
                   self._sh(stream), flags=flags)

    def root_lnl_psr(self, x, n, out, freq=None, wgt=None, scaler_sums=None, site_lnl=None, states=4,
                     stream=None):
        """Root lnL of a per-site-rate CLV into `out` (float64 device tensor,
        1 element); plfx.h section 11."""
        self._root_lnl(True, False, states, x, n, out, None, freq, wgt, scaler_sums, site_lnl, stream)

    def root_lnl_psr_gen(self, states, x, n, out, freq=None, wgt=None, scaler_sums=None, site_lnl=None,
                         stream=None):
        """root_lnl_psr() with a state count (plfx.h section 11b): states
        values per site, freq None = 1/states each."""
        self._root_lnl(True, True, states, x, n, out, None, freq, wgt, scaler_sums, site_lnl, stream)

    def edge_sumtable_psr(self, x2, sumtab, n, x1=None, tip1=None, tipvec=None, states=4, stream=None):
        """sumtab = x1 * x2 over 4*n values (plfx.h section 11); side 1 is the
        dense CLV x1 or the uint8 codes tip1 with the eigen-convention table."""
        self._edge_sumtable(True, False, states, x2, sumtab, n, x1, tip1, tipvec, stream)

    def edge_sumtable_psr_gen(self, states, x2, sumtab, n, x1=None, tip1=None, tipvec=None, stream=None):
        """edge_sumtable_psr() with a state count (plfx.h section 11c): states
        4 is edge_sumtable_psr() itself; with states 20 the CLVs and the table
        hold 20*n values and tip1 holds protein codes (row min(code, 23) of the
        PROT_CODES x 20 eigen-convention tipvec)."""
        self._edge_sumtable(True, True, states, x2, sumtab, n, x1, tip1, tipvec, stream)

    def edge_sumtables_psr(self, edges, n, tipvec=None, states=4, stream=None):
        """The sum tables of many per-site-rate branches in one call
        (plfx_edge_sumtable_psr_batch).  edges: a list of dicts with x2,
        sumtab and exactly one of x1 / tip1, as edge_sumtable_psr's arguments;
        every table of the call must be apart from every other table and
        from every input, inputs may repeat."""
        self._edge_sumtables_psr(False, states, edges, n, tipvec, stream)

    def edge_sumtables_psr_gen(self, states, edges, n, tipvec=None, stream=None):
        """edge_sumtables_psr() with a state count (plfx_edge_sumtable_psr_batch_gen):
        every CLV and table holds states*n values."""
        self._edge_sumtables_psr(True, states, edges, n, tipvec, stream)

    def _edge_sumtables_psr(self, gen, states, edges, n, tipvec, stream):
        import torch

        S = self._psr_states(gen, states)
        if isinstance(edges, dict):
            edges = [edges]
        n = int(n)
        dt = edges[0]["sumtab"].dtype if edges and edges[0].get("sumtab") is not None else torch.float64
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        arr = (PsrEdge * max(1, len(edges)))()
        for i, e in enumerate(edges):
            for k in ("x1", "x2", "sumtab"):
                _tensor(e.get(k), k, dt, S * n, optional=True)
            _tensor(e.get("tip1"), "tip1", torch.uint8, n, optional=True)
            arr[i] = PsrEdge(*(_ptr(e.get(k)) for k in ("tip1", "x1", "x2", "sumtab")))
        self._call("plfx_edge_sumtable_psr_batch", dt, S, True, gen, arr, len(edges), n, self._tipvec(tipvec, dt, S),
                   self._sh(stream))

    def edge_derivatives_psr(self, sumtab, n, eigen, rates, rate_cat, t, out, wgt=None, scaler_sums=None,
                             site_lnl=None, states=4, stream=None):
        """out (float64 device tensor, 3 elements) = lnL, d lnL/dt, d2 lnL/dt2 of
        the per-site-rate branch whose sum table is `sumtab`, at the device
        double `t`; rates holds the ncat category rates (plfx.h section 11)."""
        self._edge_derivatives(True, False, states, sumtab, n, eigen, rates, rate_cat, wgt, t, out, scaler_sums,
                               site_lnl, stream)

    def edge_derivatives_psr_gen(self, states, sumtab, n, eigen, rates, rate_cat, t, out, wgt=None,
                                 scaler_sums=None, site_lnl=None, stream=None):
        """edge_derivatives_psr() with a state count (plfx.h section 11c): with
        states 20 the table holds 20*n values and eigen is what
        pmatrix(states=20) takes."""
        self._edge_derivatives(True, True, states, sumtab, n, eigen, rates, rate_cat, wgt, t, out, scaler_sums,
                               site_lnl, stream)

    def optimize_branch_psr(self, sumtab, n, eigen, rates, rate_cat, t0, tmin=1e-8, tmax=10.0, max_evals=64,
                            wgt=None, states=4, stream=None):
        """optimize_branch for a per-site-rate branch (plfx_edge_optimize_psr,
        host-synchronous).  Returns (t, lnL, d1, d2, evals)."""
        return self._optimize_branch(True, False, states, sumtab, n, eigen, rates, rate_cat, wgt, t0, tmin, tmax,
                                     max_evals, stream)

    def optimize_branch_psr_gen(self, states, sumtab, n, eigen, rates, rate_cat, t0, tmin=1e-8, tmax=10.0,
                                max_evals=64, wgt=None, stream=None):
        """optimize_branch_psr() with a state count (plfx_edge_optimize_psr_gen,
        host-synchronous).  Returns (t, lnL, d1, d2, evals)."""
        return self._optimize_branch(True, True, states, sumtab, n, eigen, rates, rate_cat, wgt, t0, tmin, tmax,
                                     max_evals, stream)

    def optimize_branches_psr(self, sumtabs, n, eigen, rates, rate_cat, t0, t_opt, tmin=1e-8, tmax=10.0,
                              max_evals=64, out3=None, evals=None, wgt=None, states=4, stream=None):
        """optimize_branches for per-site-rate branches, with the loop on the
        device (plfx_edge_optimize_psr_dev): asynchronous, capture-safe.
        sumtabs: device tensors of 4*n values each; rate_cat, rates as
        edge_derivatives_psr; t0, t_opt, out3, evals as optimize_branches."""
        self._optimize_branches(True, False, states, sumtabs, n, eigen, rates, rate_cat, wgt, t0, t_opt, tmin, tmax,
                                max_evals, out3, evals, stream)

    def optimize_branches_psr_gen(self, states, sumtabs, n, eigen, rates, rate_cat, t0, t_opt, tmin=1e-8,
                                  tmax=10.0, max_evals=64, out3=None, evals=None, wgt=None, stream=None):
        """optimize_branches_psr() with a state count (plfx_edge_optimize_psr_dev_gen):
        asynchronous, capture-safe; sumtabs: device tensors of states*n values each."""
        self._optimize_branches(True, True, states, sumtabs, n, eigen, rates, rate_cat, wgt, t0, t_opt, tmin, tmax,
                                max_evals, out3, evals, stream)

    # -- (13) all-branch derivatives of a per-site-rate tree ------------------
    def branch_sumtables_psr(self, states, ops, clv, pmats, root_pmat, EV, n, rate_cat, ncat, scaler_sums, workspace,
                             wgt=None, edge_scale=None, tips=None, tipvec=None, fma=False, nofuse=False,
                             stream=None):
        """The outer CLVs and the sum table of every branch of the tree that
        traverse_psr_gen(states, ops, clv, pmats, ...) has just run
        (plfx_branch_sumtables_psr, plfx.h section 13).  root_pmat: ncat *
        states^2 values, pmatrix() of the joined root length; scaler_sums: the
        traversal's (int64, one per op; may be None without edge_scale);
        workspace: a uint8 device tensor of branch_sumtables_psr_workspace()
        bytes; edge_scale: optional int64 device tensor of 2 * nops counts.
        Returns the 2 * nops sum tables, edge 2*j + s = op j's child s, as
        views of the workspace (the root op's two entries are one table),
        ready for optimize_branches_psr_gen.  nofuse: PLFX_BRANCH_NOFUSE."""
        import torch

        S = self._psr_states(True, states)
        n, ncat = int(n), int(ncat)
        dt = EV.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        top, nops, slots, tp, nslots, npmats, _ = self._traverse_args(
            ops, clv, pmats, EV, n, wgt, None, scaler_sums, tips, S, S * S * max(ncat, 1), S * S)
        _tensor(rate_cat, "rate_cat", torch.uint8, n)
        _tensor(root_pmat, "root_pmat", dt, S * S * max(ncat, 1))
        _tensor(edge_scale, "edge_scale", torch.int64, 2 * nops, optional=True)
        _tensor(workspace, "workspace", torch.uint8, 0)
        tabs = (C.c_void_p * max(1, 2 * nops))()
        flags = (FMA if fma else 0) | (BRANCH_NOFUSE if nofuse else 0)
        self._check(self._L.plfx_branch_sumtables_psr(
            self.h, F32 if dt == torch.float32 else F64, S, flags, top, nops, slots, tp, nslots, _ptr(pmats), npmats,
            _ptr(root_pmat), _ptr(EV), n, _ptr(rate_cat), ncat, _ptr(wgt), _ptr(scaler_sums),
            self._tipvec(tipvec, dt, S), _ptr(workspace), workspace.numel(), tabs, _ptr(edge_scale),
            self._sh(stream)))
        base, nbytes = workspace.data_ptr(), S * n * (4 if dt == torch.float32 else 8)
        return [workspace[(tabs[e] or base) - base:(tabs[e] or base) - base + nbytes].view(dt) for e in range(2 * nops)]

    def branch_derivatives_psr(self, states, ops, clv, pmats, root_pmat, EV, n, rate_cat, ncat, scaler_sums, workspace,
                               eigen, rates, blen, wgt=None, tips=None, tipvec=None, fma=False, nofuse=False,
                               tmin=1e-8, tmax=10.0, stream=None):
        """lnL, d lnL/dt and d2 lnL/dt2 of EVERY branch at its current length:
        branch_sumtables_psr() and then one evaluation of the device loop
        (optimize_branches_psr_gen with max_evals=1 from the current lengths,
        which stores its sums at the evaluated t, clamped into [tmin, tmax]).
        blen: the 2 * npmats branch lengths that made pmats (host values);
        edge 2*j + s has blen[2 * ops[j].pmat + s], the root op's two edges the
        sum of its two.  Returns (lnl, d1, d2), float64 device tensors of
        2 * nops, lnl with the edge's scaling correction
        edge_scale * log(2^-32) applied.  Asynchronous."""
        import torch

        rows = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 4)
        nops = rows.shape[0]
        bl = np.asarray(blen, dtype=np.float64).reshape(-1)
        t = np.array([bl[2 * rows[j, 3] + s] for j in range(nops) for s in (0, 1)], dtype=np.float64)
        if nops:
            t[-2:] = t[-2] + t[-1]
        dev = workspace.device
        scale = torch.zeros(2 * nops, dtype=torch.int64, device=dev)
        tabs = self.branch_sumtables_psr(states, ops, clv, pmats, root_pmat, EV, n, rate_cat, ncat, scaler_sums,
                                         workspace, wgt=wgt, edge_scale=scale, tips=tips, tipvec=tipvec, fma=fma,
                                         nofuse=nofuse, stream=stream)
        t0 = torch.from_numpy(t).to(dev)
        t_opt = torch.empty(2 * nops, dtype=torch.float64, device=dev)
        out3 = torch.empty(3 * 2 * nops, dtype=torch.float64, device=dev)
        self.optimize_branches_psr_gen(states, tabs, n, eigen, rates, rate_cat, t0, t_opt, tmin=tmin, tmax=tmax,
                                       max_evals=1, out3=out3, wgt=wgt, stream=stream)
        o = out3.view(-1, 3)
        return o[:, 0] + scale.to(torch.float64) * LOG_MINLIK, o[:, 1], o[:, 2]

    # -- (12) the PSR rate scan ----------------------------------------------
    def site_lnl_psr(self, x, n, site_lnl, freq=None, scalers=None, nsc=None, stride=None, states=4, stream=None):
        """Per-site lnL of a per-site-rate CLV with the site's own scaling
        correction (plfx.h section 12): site_lnl[i] = log(sum_s freq[s] x[i][s])
        + (number of rows j < nsc with scalers[j*stride + i] != 0) * log(2^-32).
        scalers: one uint8 device tensor holding the nsc rows (2-D: nsc and
        stride default to its shape; 1-D: pass both), or None for nsc = 0."""
        self._site_lnl_psr(False, states, x, n, site_lnl, freq, scalers, nsc, stride, stream)

    def site_lnl_psr_gen(self, states, x, n, site_lnl, freq=None, scalers=None, nsc=None, stride=None, stream=None):
        """site_lnl_psr() with a state count (plfx.h section 12b): states 4 is
        site_lnl_psr() itself; with states 20 x holds 20*n values and freq 20
        (None = 1/20 each)."""
        self._site_lnl_psr(True, states, x, n, site_lnl, freq, scalers, nsc, stride, stream)

    def _site_lnl_psr(self, gen, states, x, n, site_lnl, freq, scalers, nsc, stride, stream):
        import torch

        S = self._psr_states(gen, states)
        n = int(n)
        _tensor(x, "x", (torch.float32, torch.float64), S * n)
        _tensor(site_lnl, "site_lnl", torch.float64, n)
        _tensor(freq, "freq", torch.float64, S, optional=True)
        if scalers is None:
            nsc, stride = (0 if nsc is None else int(nsc)), (n if stride is None else int(stride))
        else:
            if scalers.dim() == 2 and nsc is None and stride is None:
                nsc, stride = scalers.shape
            if nsc is None or stride is None:
                raise PlfxError(ERR_INVALID, "scalers must be 2-D (nsc x stride), or pass nsc and stride")
            nsc, stride = int(nsc), int(stride)
            _tensor(scalers, "scalers", torch.uint8, max(nsc - 1, 0) * max(stride, 0) + n if nsc > 0 else 0)
        self._call("plfx_site_lnl_psr", x.dtype, S, True, gen, _ptr(x), n, _ptr(freq), _ptr(scalers), nsc, stride,
                   _ptr(site_lnl), self._sh(stream))

    def psr_rate_scan(self, ops, tips, blen, eigen, EV, tipvec, cand_rates, n, workspace, best_idx, best_lnl,
                      group=PSR_MAX_CATS, freq=None, wgt=None, all_lnl=None, out_lnl=None, states=4, stream=None):
        """The per-site rate scan (plfx.h section 12, plfx_psr_rate_scan): for
        every candidate rate the per-site lnL of the whole tree with all sites
        at that rate, and per site the best candidate.  ops: (nops, 4) int
        array of [parent, child1, child2, pmat]; tips: list (per slot) of uint8
        code tensors or None -- every leaf must be coded; blen: float64 device
        tensor of 2*npmats branch lengths; eigen as pmatrix(); EV, tipvec in
        the eigen convention (their dtype is the CLVs'); cand_rates: float64
        device tensor; workspace: a torch.uint8 device tensor of at least
        psr_rate_scan_workspace(...) bytes, 256-byte aligned; best_idx
        (int32[n]), best_lnl (float64[n]), all_lnl (float64[ncand*n], optional)
        and out_lnl (float64[1], optional) are written.  group: candidates per
        traversal (sizes the workspace; the outputs do not depend on it)."""
        self._psr_rate_scan(False, states, ops, tips, blen, eigen, EV, tipvec, cand_rates, n, workspace, best_idx,
                            best_lnl, group, freq, wgt, all_lnl, out_lnl, stream)

    def psr_rate_scan_gen(self, states, ops, tips, blen, eigen, EV, tipvec, cand_rates, n, workspace, best_idx,
                          best_lnl, group=PSR_MAX_CATS, freq=None, wgt=None, all_lnl=None, out_lnl=None, stream=None,
                          fma=False):
        """psr_rate_scan() with a state count (plfx.h section 12b): states 4 is
        psr_rate_scan() itself.  With states 20 the tips hold protein codes,
        eigen is what pmatrix(states=20) takes, EV holds 400 values, tipvec is
        the PROT_CODES x 20 eigen-convention table, freq 20 root weights, and
        the workspace is psr_rate_scan_workspace_gen(dtype, 20, ...) bytes --
        its CLVs are five times the DNA size, so `group` is what sizes it.
        fma: PLFX_FMA through plfx_psr_rate_scan_ex: every pass's traversal in
        FMA mode, as traverse_psr_gen(fma=True)."""
        self._psr_rate_scan(True, states, ops, tips, blen, eigen, EV, tipvec, cand_rates, n, workspace, best_idx,
                            best_lnl, group, freq, wgt, all_lnl, out_lnl, stream, FMA if fma else None)

    def _psr_rate_scan(self, gen, states, ops, tips, blen, eigen, EV, tipvec, cand_rates, n, workspace, best_idx,
                       best_lnl, group, freq, wgt, all_lnl, out_lnl, stream, flags=None):
        import torch

        S = self._psr_states(gen, states)
        n, group = int(n), int(group)
        dt = EV.dtype
        if dt not in (torch.float32, torch.float64):
            raise PlfxError(ERR_INVALID, f"unsupported dtype {dt}")
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 4)
        nops, nslots = ops.shape[0], len(tips)
        for s_, t in enumerate(tips):
            _tensor(t, f"tip slot {s_}", torch.uint8, n, optional=True)
        _tensor(blen, "blen", torch.float64, 0)
        if blen.numel() % 2:
            raise PlfxError(ERR_INVALID, "blen must hold whole (left, right) pairs")
        npmats, ncand = blen.numel() // 2, 0 if cand_rates is None else cand_rates.numel()
        _tensor(eigen, "eigen", torch.float64, S + 2 * S * S)
        _tensor(EV, "EV", dt, S * S)
        _tensor(cand_rates, "cand_rates", torch.float64, 0)
        _tensor(freq, "freq", torch.float64, S, optional=True)
        _check_aux(n, wgt, None, None)
        _tensor(workspace, "workspace", torch.uint8, 0)
        _tensor(best_idx, "best_idx", torch.int32, n)
        _tensor(best_lnl, "best_lnl", torch.float64, n)
        _tensor(all_lnl, "all_lnl", torch.float64, ncand * n, optional=True)
        _tensor(out_lnl, "out_lnl", torch.float64, 1, optional=True)
        top = (TravOp * max(1, nops))(*[TravOp(*map(int, r)) for r in ops])
        tp = (C.c_void_p * max(1, nslots))(*map(_ptr, tips))
        self._call("plfx_psr_rate_scan", dt, S, True, gen, top, nops, tp, nslots, _ptr(blen), npmats, _ptr(eigen),
                   _ptr(EV), self._tipvec(tipvec, dt, S), _ptr(cand_rates), ncand, group, _ptr(freq), _ptr(wgt), n,
                   _ptr(workspace), workspace.numel(), _ptr(best_idx), _ptr(best_lnl), _ptr(all_lnl), _ptr(out_lnl),
                   self._sh(stream), flags=flags)

    # -- (4) scaler reduction ----------------------------------------------
    def scaler_sum(self, scaler, wgt, out_sum, n=None, stream=None):
        import torch

        if n is None:
            n = scaler.numel()
        if scaler.dtype != torch.uint8 or out_sum.dtype != torch.int64:
            raise PlfxError(ERR_INVALID, "scaler uint8, out_sum int64")
        _check_aux(n, wgt, scaler, out_sum)
        p = _ptr
        self._check(self._L.plfx_scaler_sum(self.h, p(scaler), p(wgt), int(n), p(out_sum),
                                            self._sh(stream)))


def _stream_handle(stream, device=None):
    """None = torch's current stream ON THE CONTEXT'S DEVICE (not the current
    device's), a torch.cuda.Stream, or a raw hipStream_t int."""
    if stream is None:
        import torch

        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


def _ptr(t):
    """The address of a tensor's data as a c_void_p (None: NULL)."""
    return C.c_void_p(None if t is None else t.data_ptr())


def _nptr(a):
    """The same of a numpy array."""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _node(nd):
    """plfx_node of a node dict (absent scaler / scaler_sum: NULL)."""
    return Node(*(_ptr(nd.get(k)) for k in ("x1", "x2", "x3", "left", "right", "scaler", "scaler_sum")))


def _tensor(t, name, dtype, count, contiguous=True, optional=False):
    """Refuse (PlfxError, ERR_INVALID) a tensor argument the library would
    misread -- the C ABI sees a bare pointer: t must be a device tensor of
    `dtype` (one dtype, or a tuple of the allowed ones) with at least `count`
    elements, and contiguous where the call site demands it.  optional: None
    passes (a NULL the library takes or refuses itself)."""
    if t is None and optional:
        return
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if (t is None or t.dtype not in dtypes or t.numel() < count or not t.is_cuda
            or (contiguous and not t.is_contiguous())):
        kinds = " / ".join(str(d).replace("torch.", "") for d in dtypes)
        raise PlfxError(ERR_INVALID, f"{name} must be a {'contiguous ' if contiguous else ''}{kinds} device tensor "
                                     f"of >= {count} elements")


def _check_aux(n, wgt, scaler, scaler_sum):
    """Shapes/dtypes/devices of the optional per-site weight, scaler bytes and
    scaler-sum outputs (the C ABI cannot see tensor sizes)."""
    import torch

    _tensor(wgt, "wgt", torch.int32, n, optional=True)
    _tensor(scaler, "scaler", torch.uint8, n, optional=True)
    _tensor(scaler_sum, "scaler_sum", torch.int64, 1, contiguous=False, optional=True)


def shard(total, parts, k):
    """The reference's partition (include.h:181-189; host_mem.cpp:229): part k
    of `total` items over `parts` -> (offset, count).  Used for inner nodes
    over ranks (BASELINE configs[3]) and sites over instances."""
    off, cnt = C.c_uint64(0), C.c_uint64(0)
    rc = load().plfx_shard(int(total), int(parts), int(k), C.byref(off), C.byref(cnt))
    if rc != OK:
        raise PlfxError(rc, f"plfx_shard({total}, {parts}, {k}): the reference's split underflows")
    return int(off.value), int(cnt.value)


def gen_hostmem(n, dtype=np.float64, seed=20250117, wgt=True):
    """host_mem.cpp:179-209 inputs (std::mt19937 + uniform_real_distribution,
    x1 x 1e-12 on every 4th site, wgt = 1) with a fixed seed, generated by
    libplfx (plfx_gen_hostmem).  Returns dict(EV, left, right, x1, x2, wgt)."""
    dt = np.dtype(dtype)
    out = dict(EV=np.empty(16, dt), left=np.empty(64, dt), right=np.empty(64, dt),
               x1=np.empty(16 * n, dt), x2=np.empty(16 * n, dt),
               wgt=np.empty(n, np.int32) if wgt else None)
    p = _nptr
    rc = load().plfx_gen_hostmem(F32 if dt == np.float32 else F64, int(seed), int(n), p(out["EV"]),
                                 p(out["left"]), p(out["right"]), p(out["x1"]), p(out["x2"]),
                                 p(out["wgt"]))
    if rc != OK:
        raise PlfxError(rc, "plfx_gen_hostmem")
    return out


def swemu_instance_run(in_left, in_right, out_clv, out_scaler, alignment_sites, window_size,
                       layout, aie_type=AIE_WINDOW):
    """The sw_emu target (plfx.h section 5b, BASELINE configs[0]): one
    accelerator instance emulated on the CPU as its dataflow -- movers, AIE
    lanes, s2mm -- over the whole padded host instance buffers.  No GPU."""
    dt = in_left.dtype
    if dt not in (np.float32, np.float64) or in_right.dtype != dt or out_clv.dtype != dt:
        raise PlfxError(ERR_INVALID, "instance buffers must share a float dtype")
    for a in (in_left, in_right, out_clv, out_scaler):
        if a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous):
            raise PlfxError(ERR_INVALID, "instance buffers must be C-contiguous numpy arrays")
    n = int(alignment_sites)
    tb = Testbench(n, 1, window_size or 1024, layout, aie_type)
    if in_left.size < tb.instance_elements_left() or in_right.size < tb.instance_elements_right() \
            or out_clv.size < 16 * n or (out_scaler is not None and out_scaler.size < n):
        raise PlfxError(ERR_INVALID, "buffers smaller than the padded instance")
    p = _nptr
    rc = load().plfx_swemu_instance_run(p(in_left), p(in_right), p(out_clv), p(out_scaler), n,
                                        int(window_size), int(layout), int(aie_type),
                                        F32 if dt == np.float32 else F64)
    if rc != OK:
        raise PlfxError(rc, "plfx_swemu_instance_run")


_default_ctx = None


def _dbl(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _host_check(rc, what):
    if rc != OK:
        raise PlfxError(rc, what)


def model_eigen(exch, freqs):
    """Eigensystem of a time-reversible model (plfx.h (9)).  Returns a float64
    array lambda[S] | V[S*S] | Vinv[S*S] (the device pmatrix input)."""
    L = load()
    f, fp = _dbl(freqs)
    S = f.size
    e, ep = _dbl(exch)
    if e.size != S * (S - 1) // 2:
        raise PlfxError(ERR_INVALID, "exch needs S(S-1)/2 values")
    out, op = _dbl(np.zeros(S + 2 * S * S))
    _host_check(L.plfx_model_eigen(S, ep, fp, op), "model_eigen")
    return out


def gamma_rates(alpha, ncat=4, median=False):
    """Yang (1994) discrete-Gamma category rates (plfx.h (9))."""
    L = load()
    out, op = _dbl(np.zeros(ncat))
    _host_check(L.plfx_gamma_rates(float(alpha), int(ncat), 1 if median else 0, op), "gamma_rates")
    return out


def _scan_dtype(dtype):
    if not isinstance(dtype, int):
        name = str(dtype).replace("torch.", "")
        if name not in ("float32", "float64"):
            name = np.dtype(dtype).name
        dtype = {"float32": F32, "float64": F64}.get(name, -1)
    return int(dtype)


def psr_rate_scan_workspace(dtype, nops, ntips, npmats, n, group=PSR_MAX_CATS):
    """Bytes of the workspace psr_rate_scan() needs (plfx.h section 12).  dtype:
    F32 / F64, a numpy dtype or a torch dtype; ntips: the coded tips."""
    out = C.c_size_t(0)
    _host_check(load().plfx_psr_rate_scan_workspace(_scan_dtype(dtype), int(nops), int(ntips), int(npmats), int(n),
                                                    int(group), C.byref(out)), "psr_rate_scan_workspace")
    return int(out.value)


def branch_sumtables_psr_workspace(dtype, states, nops, n):
    """Bytes of the workspace Context.branch_sumtables_psr() needs (plfx.h
    section 13): the outer CLVs, the 2 * nops - 1 tables and the counters.
    dtype: F32 / F64, a numpy dtype or a torch dtype."""
    out = C.c_size_t(0)
    _host_check(load().plfx_branch_sumtables_psr_workspace(_scan_dtype(dtype), int(states), int(nops), int(n),
                                                           C.byref(out)), "branch_sumtables_psr_workspace")
    return int(out.value)


def branch_pair_sites_per_lane(dtype):
    """Sites per lane and trip of the fused sibling-pair kernel (plfx_branch_pair_sites_per_lane)."""
    return int(load().plfx_branch_pair_sites_per_lane(_scan_dtype(dtype)))


def psr_rate_scan_workspace_gen(dtype, states, nops, ntips, npmats, n, group=PSR_MAX_CATS):
    """psr_rate_scan_workspace() with a state count (plfx.h section 12b): what
    psr_rate_scan_gen(states, ...) needs.  With states 20 the CLVs are five
    times the DNA size; `group` is what sizes the workspace."""
    out = C.c_size_t(0)
    _host_check(load().plfx_psr_rate_scan_workspace_gen(_scan_dtype(dtype), int(states), int(nops), int(ntips),
                                                        int(npmats), int(n), int(group), C.byref(out)),
                "psr_rate_scan_workspace_gen")
    return int(out.value)


def psr_categorize(cand_rates, best_idx, wgt=None, max_cats=PSR_MAX_CATS):
    """The scan's best candidates binned into at most max_cats categories
    (plfx.h section 12, plfx_psr_categorize), on numpy arrays.  Returns
    (rate_cat uint8[n], cat_rates float64[ncat], scale): cat_rates are the kept
    candidates times scale, so that the weighted mean rate is 1."""
    r, rp = _dbl(cand_rates)
    idx = np.ascontiguousarray(best_idx, dtype=np.int32).reshape(-1)
    w = None if wgt is None else np.ascontiguousarray(wgt, dtype=np.int32).reshape(-1)
    if w is not None and w.size != idx.size:
        raise PlfxError(ERR_INVALID, "wgt must have one entry per site")
    max_cats = int(max_cats)
    cat = np.zeros(idx.size, np.uint8)
    rates, ratesp = _dbl(np.zeros(max(max_cats, 1)))
    ncat, scale = C.c_int(0), C.c_double(0.0)
    _host_check(load().plfx_psr_categorize(rp, r.size, _nptr(idx), _nptr(w), idx.size, max_cats, _nptr(cat), ratesp,
                                           C.byref(ncat), C.byref(scale)), "psr_categorize")
    return cat, rates[:ncat.value].copy(), float(scale.value)


def psr_site_order(rate_cat, ncat):
    """The stable order of the sites by clamped category (plfx.h section 11b,
    plfx_psr_site_order): an int64 permutation perm with perm[j] = the site
    that goes to position j.  Apply it to every tip's codes, wgt and rate_cat
    once, after psr_categorize(): the protein PSR node is fast on sorted
    sites.  rate_cat: host uint8 array."""
    cat = np.ascontiguousarray(rate_cat)
    if cat.dtype != np.uint8 or cat.ndim != 1:
        raise PlfxError(ERR_INVALID, "rate_cat must be a one-dimensional uint8 array")
    perm = np.empty(cat.size, np.int64)
    _host_check(load().plfx_psr_site_order(_nptr(cat), cat.size, int(ncat), _nptr(perm)), "psr_site_order")
    return perm


def model_ev(eigen, states, convention=PMAT_STATE):
    L = load()
    e, ep = _dbl(eigen)
    out, op = _dbl(np.zeros(states * states))
    _host_check(L.plfx_model_ev(states, convention, ep, op), "model_ev")
    return out


def model_root_weights(eigen, freqs, convention=PMAT_STATE):
    L = load()
    f, fp = _dbl(freqs)
    e, ep = _dbl(eigen)
    out, op = _dbl(np.zeros(f.size))
    _host_check(L.plfx_model_root_weights(f.size, convention, ep, fp, op), "model_root_weights")
    return out


def model_tip_vectors(eigen=None, convention=PMAT_STATE, states=4):
    """16 x S tip vectors for the tip paths (plfx.h (9))."""
    L = load()
    out, op = _dbl(np.zeros(16 * states))
    if eigen is None:
        ep = C.cast(None, C.POINTER(C.c_double))
    else:
        e, ep = _dbl(eigen)
    _host_check(L.plfx_model_tip_vectors(states, convention, ep, op), "model_tip_vectors")
    return out


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def plf(x1_start, x2_start, x3_start, EV, n, left, right, wgt=None):
    """Module-level drop-in for the reference plf() (app/src/plf.h:1-5) on the
    default context.  Returns scalerIncrement."""
    return default_context().plf(x1_start, x2_start, x3_start, EV, n, left, right, wgt)


class Testbench:
    """testbench_info (app/src/include.h:150-266) via the C ABI (64-bit)."""

    def __init__(self, alignment_sites, parallel_instances=1, window_size=1024,
                 layout=LAYOUT_SEPARATE, aie_type=AIE_WINDOW):
        self._L = load()
        self.t = _TB(int(alignment_sites), int(parallel_instances), int(window_size), int(layout),
                     int(aie_type))

    def __getattr__(self, name):
        f = getattr(self._L, f"plfx_tb_{name}", None)
        if f is None:
            raise AttributeError(name)
        if len(f.argtypes) == 2:
            return lambda k=-1: int(f(C.byref(self.t), int(k)))
        return lambda: int(f(C.byref(self.t)))

    def pack_instance(self, k, EV, left, right, x1, x2):
        dt = np.asarray(x1).dtype
        L = np.empty(self.instance_elements_left(), dt)
        R = np.empty(self.instance_elements_right(), dt)
        keep = [np.ascontiguousarray(a, dt) for a in (EV, left, right, x1, x2)]
        rc = self._L.plfx_pack_instance(C.byref(self.t), int(k), F32 if dt == np.float32 else F64,
                                        *[a.ctypes.data_as(C.c_void_p) for a in keep],
                                        L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p))
        if rc != OK:
            raise PlfxError(rc, "plfx_pack_instance failed")
        return L, R
