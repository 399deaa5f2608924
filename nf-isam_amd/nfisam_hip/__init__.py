"""ctypes binding of the C ABI in include/nfisam_hip.h (libnfisam_hip.so, built from
nf-isam_amd/csrc by `make -C nf-isam_amd/csrc` or `__graft_entry__.build()`).

PyTorch is used here only as plumbing: device memory (tensors), streams.  Every compute entry
point goes to the hand-written gfx950 kernels; there is NO CPU or eager-PyTorch fallback — if
the library is missing or the tensors are not on a ROCm device the calls raise.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnfisam_hip.so")
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

OK, ERR_ARG, ERR_LAUNCH, ERR_DOMAIN, ERR_NO_DEVICE, ERR_STALL = 0, 1, 2, 3, 4, 5

EXPORTS = [
    "nfisam_abi_version", "nfisam_last_hip_error", "nfisam_nsf_supported", "nfisam_nsf_param_count",
    "nfisam_nsf_kparam_count", "nfisam_nsf_layout_map", "nfisam_nsf_forward", "nfisam_nsf_inverse",
    "nfisam_nsf_backward", "nfisam_nsf_train_step", "nfisam_nsf_train_loop", "nfisam_nsf_train_plan_create",
    "nfisam_nsf_train_plan_run", "nfisam_nsf_train_plan_destroy", "nfisam_rqs", "nfisam_nsf_posterior_walk", "nfisam_nsf_grad_workspace_count", "nfisam_nsf_train_gradient", "nfisam_nsf_train_chains", "nfisam_nsf_train_gradient_part",
    "nfisam_nsf_train_plan_begin", "nfisam_nsf_train_plan_enqueue", "nfisam_nsf_train_plan_peek", "nfisam_nsf_train_plan_stream",
    "nfisam_nsf_train_plan_end", "nfisam_nsf_train_plan_xcd_span", "nfisam_nsf_train_plan_kernel_ms", "nfisam_nsf_train_plan_create_validated", "nfisam_nsf_train_plan_feed", "nfisam_nsf_train_plan_enqueued", "nfisam_nsf_train_plan_refill",
    "nfisam_normalize_columns", "nfisam_simulate_clique", "nfisam_nsf_train_plan_launch_async",
    "nfisam_nsf_posterior_log_density", "nfisam_factor_graph_log_density",
    "nfisam_sample_mmd", "nfisam_sample_mmd_scratch_count",
    "nfisam_sample_mmd_perm", "nfisam_sample_mmd_perm_scratch_count",
    "nfisam_sample_moments", "nfisam_sample_quantiles",
    "nfisam_sample_modes", "nfisam_sample_modes_merge",
    "nfisam_factor_graph_score", "nfisam_factor_graph_score_scratch_count",
    "nfisam_factor_graph_hvp", "nfisam_factor_graph_hvp_scratch_count",
    "nfisam_sample_ksd", "nfisam_sample_ksd_scratch_count",
    "nfisam_sample_svgd", "nfisam_sample_svgd_scratch_count", "nfisam_sample_step",
    "nfisam_sample_propose", "nfisam_sample_accept", "nfisam_sample_accept_scratch_count",
    "nfisam_chain_record", "nfisam_chain_finish", "nfisam_chain_state_count",
    "nfisam_sample_knn", "nfisam_sample_ball_count",
    "nfisam_sample_density",
    "nfisam_sample_trajectory_error", "nfisam_sample_trajectory_rpe", "nfisam_sample_trajectory_scratch_count",
    "nfisam_sample_sliced_transport",
]


class HipLibraryMissing(ImportError):
    pass


class TrainState(C.Structure):
    _fields_ = [("step", C.c_int32), ("stop", C.c_int32), ("have_avg", C.c_int32), ("loss_avg", C.c_float),
                ("domain_err", C.c_int32), ("reserved", C.c_int32 * 3)]


class AdamCfg(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("max_iters", C.c_int32), ("average_window", C.c_int32), ("loss_delta_tol", C.c_float),
                ("reserved", C.c_int32)]


class Clique(C.Structure):
    _fields_ = [("x", C.c_void_p), ("kparams", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p),
                ("kgrad", C.c_void_p), ("iter_loss", C.c_void_p), ("state", C.c_void_p),
                ("n", C.c_int32), ("D", C.c_int32)]


class Validation(C.Structure):
    _fields_ = [("x_val", C.c_void_p), ("logprob", C.c_void_p), ("val_loss", C.c_void_p), ("n_val", C.c_int32),
                ("reserved", C.c_int32)]


class PostClique(C.Structure):
    _fields_ = [("kparams", C.c_void_p), ("mean", C.c_void_p), ("std", C.c_void_p), ("circular", C.c_void_p),
                ("D_model", C.c_int32), ("n_obs", C.c_int32), ("n_sep", C.c_int32), ("n_frontal", C.c_int32),
                ("obs_off", C.c_int32), ("sep_off", C.c_int32), ("front_off", C.c_int32), ("reserved", C.c_int32)]


class FactorTerm(C.Structure):
    _fields_ = [("code", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("k", C.c_int32), ("cand", C.c_int32 * 4),
                ("p", C.c_double * 16)]


assert C.sizeof(TrainState) == 32 and C.sizeof(AdamCfg) == 32 and C.sizeof(Clique) == 64 and C.sizeof(PostClique) == 64
assert C.sizeof(FactorTerm) == 160


class MmdBlock(C.Structure):
    _fields_ = [("col_off", C.c_int32), ("d", C.c_int32), ("inv_two_sigma2", C.c_double)]


assert C.sizeof(MmdBlock) == 16


class TransportBlock(C.Structure):
    _fields_ = [("col_off", C.c_int32), ("d", C.c_int32), ("n_dirs", C.c_int32), ("reserved", C.c_int32),
                ("dir_off", C.c_int64), ("out_off", C.c_int64)]


assert C.sizeof(TransportBlock) == 32


class MomentBlock(C.Structure):
    _fields_ = [("col_off", C.c_int32), ("d", C.c_int32), ("cov_off", C.c_int64)]


assert C.sizeof(MomentBlock) == 16
MOMENTS_MAX_D, QUANTILE_MAX_N = 16, 16384        # NFISAM_MOMENTS_MAX_D, NFISAM_QUANTILE_MAX_N
MODES_MAX_D, MODES_MAX_MODES = 16, 32            # NFISAM_MODES_MAX_D, NFISAM_MODES_MAX_MODES

_lib = None


def build(force=False):
    """Compile the shared library for gfx950 with hipcc (works without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-s"] + (["-B"] if force else []))
    else:
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                "libnfisam_hip.so not found at %s — build it with `make -C %s` (needs hipcc). "
                "There is no CPU fallback for the NF-iSAM flow hot path." % (LIB_PATH, CSRC))
        _lib = C.CDLL(LIB_PATH)
        _lib.nfisam_nsf_param_count.restype = C.c_size_t
        _lib.nfisam_nsf_kparam_count.restype = C.c_size_t
        _lib.nfisam_nsf_grad_workspace_count.restype = C.c_size_t
        _lib.nfisam_nsf_train_plan_stream.restype = C.c_void_p
        _lib.nfisam_nsf_train_plan_enqueued.restype = C.c_long
        _lib.nfisam_sample_mmd_scratch_count.restype = C.c_size_t
        _lib.nfisam_sample_mmd_perm_scratch_count.restype = C.c_size_t
        _lib.nfisam_factor_graph_score_scratch_count.restype = C.c_size_t
        _lib.nfisam_factor_graph_hvp_scratch_count.restype = C.c_size_t
        _lib.nfisam_sample_ksd_scratch_count.restype = C.c_size_t
        _lib.nfisam_sample_svgd_scratch_count.restype = C.c_size_t
        _lib.nfisam_sample_accept_scratch_count.restype = C.c_size_t
        _lib.nfisam_chain_state_count.restype = C.c_size_t
        _lib.nfisam_sample_trajectory_scratch_count.restype = C.c_size_t
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_longlong               # (two 64-bit counts among the ints: spelled out)
        _lib.nfisam_sample_sliced_transport.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, i64, i32,
                                                        vp, i64, vp]
        _lib.nfisam_sample_sliced_transport.restype = C.c_int
        for name in EXPORTS:
            getattr(_lib, name)   # raises AttributeError if the ABI is incomplete
    return _lib


class DomainError(RuntimeError):
    """NFISAM_ERR_DOMAIN: a kernel saw a non-finite loss (the reference raises / asserts at src/flows/utils.py:74-76,133)."""


class PersistentStall(RuntimeError):
    """NFISAM_ERR_STALL: a chunk-persistent training launch gave up waiting for one of its own blocks (somebody else held
    its place on the device).  NOT a numerical failure: the fit is incomplete; re-run it from its initial state -- the
    library keeps to one launch per iteration for the rest of the process."""


def _check(rc, what):
    if rc == OK:
        return
    msg = {ERR_ARG: "invalid argument / unsupported (K,H)", ERR_LAUNCH: "HIP launch failure (hip error %d)" %
           lib().nfisam_last_hip_error(), ERR_DOMAIN: "numerical domain error", ERR_NO_DEVICE: "no gfx950 device",
           ERR_STALL: "a chunk-persistent training launch stalled (a block never became resident)"}
    if rc == ERR_ARG:
        raise ValueError("%s: %s" % (what, msg[rc]))
    if rc == ERR_DOMAIN:
        raise DomainError("%s: %s" % (what, msg[rc]))
    if rc == ERR_STALL:
        raise PersistentStall("%s: %s" % (what, msg[rc]))
    raise RuntimeError("%s: %s" % (what, msg.get(rc, "error %d" % rc)))


def supported(K, H):
    return bool(lib().nfisam_nsf_supported(int(K), int(H)))


def param_count(D, K, H):
    return int(lib().nfisam_nsf_param_count(int(D), int(K), int(H)))


def kparam_count(D, K, H):
    return int(lib().nfisam_nsf_kparam_count(int(D), int(K), int(H)))


_map_cache = {}


def layout_map(D, K, H):
    """np.int32[kparam_count]: index into the reference-order blob, -1 for padding."""
    key = (int(D), int(K), int(H))
    if key not in _map_cache:
        m = np.empty(kparam_count(*key), dtype=np.int32)
        _check(lib().nfisam_nsf_layout_map(key[0], key[1], key[2], m.ctypes.data_as(C.c_void_p)), "layout_map")
        _map_cache[key] = m
    return _map_cache[key]


_tmap_cache = {}


def _torch_maps(D, K, H, device):
    key = (int(D), int(K), int(H), str(device))
    if key not in _tmap_cache:
        m = layout_map(D, K, H)
        valid = torch.from_numpy((m >= 0))
        src = torch.from_numpy(np.where(m >= 0, m, 0).astype(np.int64))
        kidx = torch.from_numpy(np.nonzero(m >= 0)[0].astype(np.int64))
        tidx = torch.from_numpy(m[m >= 0].astype(np.int64))
        _tmap_cache[key] = (valid.to(device).to(torch.float32), src.to(device), kidx.to(device), tidx.to(device))
    return _tmap_cache[key]


class _Staging:
    """Pinned staging ring for the many SMALL host -> device copies of the pipeline (clique tables, observation rows,
    normalisation constants).  A copy from pageable memory blocks the host until the stream has drained in front of it
    (measured: 30-200 us each, 1.6 s of a 17 s eight-replica Plaza1 run); from the ring it is asynchronous.  One ring per
    (thread, stream): a chunk is reused only after the event recorded behind its last copy has fired."""
    CHUNK, CHUNKS = 1 << 16, 8

    def __init__(self):
        self.buf = torch.empty(self.CHUNK * self.CHUNKS, dtype=torch.uint8).pin_memory()
        self.host = self.buf.numpy()
        self.events = [None] * self.CHUNKS
        self.cur, self.off = 0, 0

    def put(self, raw: np.ndarray, device) -> "torch.Tensor":
        n = raw.size
        if self.off + n > self.CHUNK:
            ev = self.events[self.cur] or torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.events[self.cur] = ev
            self.cur, self.off = (self.cur + 1) % self.CHUNKS, 0
            if self.events[self.cur] is not None:
                self.events[self.cur].synchronize()
        a = self.cur * self.CHUNK + self.off
        self.host[a:a + n] = raw
        self.off += (n + 63) & ~63
        return self.buf[a:a + n].to(device, non_blocking=True)


_staging = threading.local()


def upload(*arrays, device, cached=False):
    """Small numpy arrays -> device tensors of the same dtype and shape, ONE asynchronous copy for all of them on the
    current stream (each array starts 64-byte aligned in the transfer).  The result is ordered behind the copy on THAT
    stream only: a tensor that is kept and later used on other streams (`cached=True`: a model's circular flags, tables that
    outlive the call) is copied the plain way instead -- from pageable memory, host-synchronous, complete when the call
    returns and therefore safe on any stream.  A non-CUDA `device` never goes through the pinned ring (a `.to` of a pinned
    slice onto the CPU would alias the ring)."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    if not arrays:
        return []
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 63) & ~63
    raw = np.zeros(max(total, 1), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        raw[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    if total > _Staging.CHUNK or cached or not torch.cuda.is_available() or torch.device(device).type != "cuda":
        dev = torch.from_numpy(raw).to(device)
    else:
        rings = _staging.__dict__.setdefault("rings", {})
        key = torch.cuda.current_stream().cuda_stream
        ring = rings.get(key)
        if ring is None:
            ring = rings[key] = _Staging()
        dev = ring.put(raw, device)
    out = []
    for a, o in zip(arrays, offs):
        out.append(dev[o:o + a.nbytes].view(_TORCH_OF[a.dtype.type]).reshape(a.shape))
    return out


_TORCH_OF = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8, np.int64: torch.int64,
             np.float64: torch.float64, np.bool_: torch.bool}


def pack(blob, D, K, H, L=1):
    """reference-order parameters [L*P] -> kernel layout [L*Pk] (same device/dtype float32)."""
    P, Pk = param_count(D, K, H), kparam_count(D, K, H)
    blob = blob.reshape(L, P)
    valid, src, _, _ = _torch_maps(D, K, H, blob.device)
    out = blob[:, src] * (valid if blob.dtype == torch.float32 else valid.to(blob.dtype))
    return out.reshape(L * Pk).contiguous()


def unpack(kblob, D, K, H, L=1):
    """kernel layout [L*Pk] -> reference-order parameters [L*P]."""
    P, Pk = param_count(D, K, H), kparam_count(D, K, H)
    kblob = kblob.reshape(L, Pk)
    _, _, kidx, tidx = _torch_maps(D, K, H, kblob.device)
    out = torch.empty(L, P, dtype=kblob.dtype, device=kblob.device)
    out[:, tidx] = kblob[:, kidx]
    return out.reshape(L * P)


def _dev(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on a ROCm device (no CPU path exists)" % name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s" % (name, dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """Raw handle of torch's current stream (what the C ABI takes).  `torch.cuda.current_stream()` builds a Stream object per
    call (2.7 us); the raw-handle lookup is 0.4 us (scripts/exp/stream_call_cost.py) -- it sits inside every launch of this module."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stride(kparams, D, K, H, L, model_D):
    """size_t layer stride for a (possibly truncated) evaluation; validates the blob size."""
    md = D if model_D is None else int(model_D)
    if md < D:
        raise ValueError("model_D=%d is smaller than the evaluated dimension %d" % (md, D))
    if kparams.numel() != L * kparam_count(md, K, H):
        raise ValueError("kparams has %d elements, expected %d" % (kparams.numel(), L * kparam_count(md, K, H)))
    return C.c_size_t(0 if md == D else kparam_count(md, K, H))


def forward(x, kparams, K, H, B, L=1, want_z=True, want_logdet=True, want_logprob=False, model_D=None):
    """x[n,D] -> (z, logdet, logprob) (None for the ones not requested)."""
    _dev(x, "x"); _dev(kparams, "kparams")
    n, D = x.shape
    stride = _stride(kparams, D, K, H, L, model_D)
    z = torch.empty_like(x) if want_z else None
    ld = torch.empty(n, dtype=torch.float32, device=x.device) if want_logdet else None
    lp = torch.empty(n, dtype=torch.float32, device=x.device) if want_logprob else None
    _check(lib().nfisam_nsf_forward(_ptr(x), _ptr(kparams), n, D, int(K), int(H), C.c_float(B), int(L), stride, _ptr(z),
                                    _ptr(ld), _ptr(lp), _stream()), "nfisam_nsf_forward")
    return z, ld, lp


def inverse(z, x_sep, kparams, K, H, B, L=1, mean=None, std=None, circular=None, want_logdet=False,
            model_D=None):
    """z[n,D-Ds], x_sep[n,Ds] raw (or None) -> x_free[n,D-Ds] (and logdet[n])."""
    _dev(z, "z"); _dev(kparams, "kparams"); _dev(x_sep, "x_sep"); _dev(mean, "mean"); _dev(std, "std")
    _dev(circular, "circular", torch.uint8)
    n, F = z.shape
    Ds = 0 if x_sep is None else x_sep.shape[1]
    D = Ds + F
    if x_sep is not None and x_sep.shape[0] != n:
        raise ValueError("x_sep and z disagree on the number of particles")
    stride = _stride(kparams, D, K, H, L, model_D)
    for t, nm in ((mean, "mean"), (std, "std"), (circular, "circular")):
        if t is not None and t.numel() < D:
            raise ValueError("%s must have at least D=%d entries" % (nm, D))
    out = torch.empty_like(z)
    ld = torch.empty(n, dtype=torch.float32, device=z.device) if want_logdet else None
    _check(lib().nfisam_nsf_inverse(_ptr(z), _ptr(x_sep), _ptr(kparams), n, D, Ds, int(K), int(H), C.c_float(B),
                                    int(L), stride, _ptr(mean), _ptr(std), _ptr(circular), _ptr(out), _ptr(ld), _stream()),
           "nfisam_nsf_inverse")
    return (out, ld) if want_logdet else out


def _rqs_call(inputs, w, h, d, inverse, left, right, bottom, top, padded):
    shape = inputs.shape
    inp = _dev(inputs.reshape(-1).contiguous().float(), "inputs")
    K = w.shape[-1]
    M = inp.numel()
    dc = K - 1 if padded else K + 1
    w = _dev(w.reshape(M, K).contiguous().float(), "unnormalized_widths")
    h = _dev(h.reshape(M, K).contiguous().float(), "unnormalized_heights")
    d = _dev(d.reshape(M, dc).contiguous().float(), "unnormalized_derivatives")
    if K * 1e-3 > 1.0:
        raise ValueError("Minimal bin width too large for the number of bins")
    out = torch.empty_like(inp); lad = torch.empty_like(inp)
    _check(lib().nfisam_rqs(_ptr(inp), _ptr(w), _ptr(h), _ptr(d), M, K, int(inverse), C.c_float(left),
                            C.c_float(right), C.c_float(bottom), C.c_float(top), int(padded), _ptr(out), _ptr(lad),
                            _stream()), "nfisam_rqs")
    return out.reshape(shape), lad.reshape(shape)


def rqs(inputs, widths, heights, derivs, inverse, tail_bound):
    """unconstrained_RQS: derivs has K-1 columns, linear tails outside [-tail_bound, tail_bound]."""
    return _rqs_call(inputs, widths, heights, derivs, inverse, -tail_bound, tail_bound, -tail_bound, tail_bound, True)


def rqs_box(inputs, widths, heights, derivs, inverse, left, right, bottom, top):
    """bounded RQS: derivs has K+1 columns."""
    return _rqs_call(inputs, widths, heights, derivs, inverse, left, right, bottom, top, False)


def backward(x, kparams, K, H, B, L=1, gz=None, gl=None, nll_mode=False, want_gx=False, model_D=None):
    """VJP of the flow.  -> (kgrad[L*Pk], gx[n,D] or None, loss_sum tensor[1] or None)."""
    _dev(x, "x"); _dev(kparams, "kparams"); _dev(gz, "gz"); _dev(gl, "gl")
    n, D = x.shape
    stride = _stride(kparams, D, K, H, L, model_D)
    kgrad = torch.zeros_like(kparams)
    gx = torch.empty_like(x) if want_gx else None
    loss = torch.zeros(1, dtype=torch.float32, device=x.device) if nll_mode else None
    _check(lib().nfisam_nsf_backward(_ptr(x), _ptr(kparams), n, D, int(K), int(H), C.c_float(B), int(L), stride, _ptr(gz),
                                     _ptr(gl), int(bool(nll_mode)), _ptr(kgrad), _ptr(gx), _ptr(loss), _stream()),
           "nfisam_nsf_backward")
    return kgrad, gx, loss


class TrainBatch:
    """Device-resident training state of a batch of independent cliques (one flow each).

    Mirrors what NFiSAM.fit_clique_density_model keeps per clique (model parameters, Adam
    moments, per-iteration loss vector; src/slam/NFiSAM.py:418-447) but for many cliques at
    once, so that one launch covers grid.y = clique."""

    def __init__(self, xs, kparams, K, H, B, L, lr, max_iters, average_window=50, loss_delta_tol=1e-2,
                 beta1=0.9, beta2=0.999, eps=1e-8, early_stop=True, x_val=None, validation_interval=10, slower_stop_rate=2.0):
        """x_val (one held-out batch per clique): the plan stops by the reference's hold-out rule (NFiSAM.py:452-468,
        nfisam_nsf_train_plan_create_validated) instead of the window rule; `val_loss[c]` then records every evaluation."""
        if len(xs) != len(kparams) or len(xs) == 0:
            raise ValueError("need one parameter blob per clique batch")
        self.x_val = None
        if x_val is not None:
            if len(x_val) != len(xs) or any(v.shape[1] != x.shape[1] or v.shape[0] < 1 for v, x in zip(x_val, xs)):
                raise ValueError("need one held-out batch [n_val, D] per clique")
            self.x_val = [_dev(v, "x_val") for v in x_val]
            self.validation_interval, self.slower_stop_rate = int(validation_interval), float(slower_stop_rate)
            early_stop = False
        self.K, self.H, self.B, self.L = int(K), int(H), float(B), int(L)
        self.device = xs[0].device
        self.xs = [_dev(x, "x") for x in xs]
        self.kparams = [_dev(p, "kparams") for p in kparams]
        for x, p in zip(self.xs, self.kparams):
            if p.numel() != L * kparam_count(x.shape[1], K, H):
                raise ValueError("kparams size does not match (D,K,H,L)")
        self.m = [torch.zeros_like(p) for p in self.kparams]
        self.v = [torch.zeros_like(p) for p in self.kparams]
        self.max_n = max(x.shape[0] for x in xs)
        self.g = [torch.zeros(int(lib().nfisam_nsf_grad_workspace_count(self.max_n, x.shape[1], int(K), int(H), int(L))),
                              dtype=torch.float32, device=self.device) for x in self.xs]
        self.iter_loss = [torch.zeros(max(int(max_iters), 1), dtype=torch.float32, device=self.device) for _ in xs]
        self.states = torch.zeros(len(xs), C.sizeof(TrainState) // 4, dtype=torch.int32, device=self.device)
        self.cfg = AdamCfg(lr, beta1, beta2, eps, int(max_iters), int(average_window) if early_stop else 0,
                           loss_delta_tol, 0)
        self.nc = len(xs)
        self.max_n = max(x.shape[0] for x in xs)
        self.max_D = max(x.shape[1] for x in xs)
        self.host_desc = (Clique * self.nc)()
        for c in range(self.nc):
            d = self.host_desc[c]
            d.x = self.xs[c].data_ptr(); d.kparams = self.kparams[c].data_ptr()
            d.adam_m = self.m[c].data_ptr(); d.adam_v = self.v[c].data_ptr(); d.kgrad = self.g[c].data_ptr()
            d.iter_loss = self.iter_loss[c].data_ptr()
            d.state = self.states.data_ptr() + C.sizeof(TrainState) * c
            d.n, d.D = self.xs[c].shape
        raw = np.frombuffer(bytes(self.host_desc), dtype=np.uint8).copy()
        self.dev_desc = torch.from_numpy(raw).to(self.device)
        if self.x_val is not None:
            n_eval = max(1, int(max_iters) // max(self.validation_interval, 1))
            self.val_scratch = [torch.empty(v.shape[0], dtype=torch.float32, device=self.device) for v in self.x_val]
            self.val_loss = [torch.zeros(n_eval, dtype=torch.float32, device=self.device) for _ in self.x_val]
            self.val_desc = (Validation * self.nc)()
            for c in range(self.nc):
                q = self.val_desc[c]
                q.x_val, q.logprob, q.val_loss = self.x_val[c].data_ptr(), self.val_scratch[c].data_ptr(), self.val_loss[c].data_ptr()
                q.n_val = self.x_val[c].shape[0]

    def step(self):
        """Enqueue ONE training iteration for all cliques (no host sync)."""
        if self.nc == 1:
            rc = lib().nfisam_nsf_train_step(C.byref(self.host_desc[0]), 1, 1, self.max_n, self.max_D, self.K, self.H,
                                             C.c_float(self.B), self.L, C.byref(self.cfg), _stream())
        else:
            rc = lib().nfisam_nsf_train_step(C.c_void_p(self.dev_desc.data_ptr()), self.nc, 0, self.max_n, self.max_D,
                                             self.K, self.H, C.c_float(self.B), self.L, C.byref(self.cfg), _stream())
        _check(rc, "nfisam_nsf_train_step")

    def chains(self):
        """Launches a training plan issues per iteration for this batch (parallel graph branches; 1 = not split)."""
        return int(lib().nfisam_nsf_train_chains(self.nc, self.max_n, self.max_D, self.K, self.H, self.L))

    def gradient_part(self, chain, n_chains, stream=None):
        """Launch `chain` of `n_chains` of the gradient half of an iteration, on `stream` (default: the current one)."""
        st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
        if self.nc == 1:
            rc = lib().nfisam_nsf_train_gradient_part(C.byref(self.host_desc[0]), 1, 1, self.max_n, self.max_D, self.K, self.H,
                                                      C.c_float(self.B), self.L, int(chain), int(n_chains), st)
        else:
            rc = lib().nfisam_nsf_train_gradient_part(C.c_void_p(self.dev_desc.data_ptr()), self.nc, 0, self.max_n, self.max_D,
                                                      self.K, self.H, C.c_float(self.B), self.L, int(chain), int(n_chains), st)
        _check(rc, "nfisam_nsf_train_gradient_part")

    def gradient_only(self):
        """Enqueue only the gradient kernel of an iteration (no Adam, no bookkeeping)."""
        if self.nc == 1:
            rc = lib().nfisam_nsf_train_gradient(C.byref(self.host_desc[0]), 1, 1, self.max_n, self.max_D, self.K,
                                                 self.H, C.c_float(self.B), self.L, _stream())
        else:
            rc = lib().nfisam_nsf_train_gradient(C.c_void_p(self.dev_desc.data_ptr()), self.nc, 0, self.max_n,
                                                 self.max_D, self.K, self.H, C.c_float(self.B), self.L, _stream())
        _check(rc, "nfisam_nsf_train_gradient")

    def prepare(self, use_graph=True, timing=False, span=False):
        """Validate descriptors and (optionally) capture + instantiate the hipGraph of one chunk of
        iterations.  One-time set-up; `run` calls it on first use.  `timing`: the graph carries two timing events around
        the chunk's training launches (`kernel_ms`; measurement only).  `span`: the plan also gets the window-spanning graph
        that `launch_async` needs (single-clique plans)."""
        if getattr(self, "_plan", None) is not None and self._plan_graph == bool(use_graph) and (not timing or getattr(self, "_plan_timing", False)) \
                and (not span or getattr(self, "_plan_span", False)):
            return
        self._plan_timing = bool(timing) and bool(use_graph)
        self._plan_span = (bool(span) or getattr(self, "_plan_span", False)) and bool(use_graph) and not self._plan_timing
        self.close()
        plan = C.c_void_p(0)
        dev_desc = C.c_void_p(self.dev_desc.data_ptr()) if self.nc > 1 else None
        if self.x_val is not None:
            rc = lib().nfisam_nsf_train_plan_create_validated(self.host_desc, dev_desc, self.nc, self.K, self.H, C.c_float(self.B), self.L,
                                                              C.byref(self.cfg), self.val_desc, self.validation_interval,
                                                              C.c_float(self.slower_stop_rate), int(bool(use_graph)) | (2 if self._plan_timing else 0) | (4 if self._plan_span else 0), C.byref(plan))
        else:
            rc = lib().nfisam_nsf_train_plan_create(self.host_desc, dev_desc, self.nc, self.K, self.H, C.c_float(self.B), self.L,
                                                    C.byref(self.cfg), int(bool(use_graph)) | (2 if self._plan_timing else 0) | (4 if self._plan_span else 0), C.byref(plan))
        _check(rc, "nfisam_nsf_train_plan_create")
        self._plan, self._plan_graph = plan, bool(use_graph)

    def run(self, use_graph=True):
        """Run until every clique stopped early or reached max_iters (the reference's
        `for i in range(flow_iterations)` loop).  Host-synchronising once per chunk.
        -> list of iterations run per clique."""
        self.prepare(use_graph)
        iters = (C.c_int32 * self.nc)()
        rc = lib().nfisam_nsf_train_plan_run(self._plan, iters, _stream())
        self.last_iters = [int(v) for v in iters]          # valid also when a clique hit a domain error
        _check(rc, "nfisam_nsf_train_plan_run")
        return self.last_iters

    def launch_async(self):
        """Enqueue the WHOLE run of a single-clique plan on the current stream as one window-spanning launch that evaluates the
        early-stop rule itself, and return at once (nfisam_nsf_train_plan_launch_async).  -> True: enqueued -- the outcome is in
        `states[0]` (step = iterations run, stop, domain_err) / `iter_loss[0]` / `kparams[0]` when the stream has drained;
        False: this plan or this moment does not allow it (call `run`)."""
        if self.nc != 1 or self.x_val is not None:
            return False
        self.prepare(True, span=True)
        rc = lib().nfisam_nsf_train_plan_launch_async(self._plan, _stream())
        if rc == ERR_ARG:
            return False
        _check(rc, "nfisam_nsf_train_plan_launch_async")
        return True

    def kernel_ms(self):
        """GPU milliseconds of the training launches of the most recent chunk replay (plans prepared with `timing=True`;
        synchronise first)."""
        ms = C.c_float(0.0)
        _check(lib().nfisam_nsf_train_plan_kernel_ms(self._plan, C.byref(ms)), "nfisam_nsf_train_plan_kernel_ms")
        return float(ms.value)

    def xcd_span(self):
        """Most XCDs one (clique, dim) group of the plan's chunk-persistent launches ran on (0: none ran; diagnostic)."""
        return int(lib().nfisam_nsf_train_plan_xcd_span(self._plan)) if getattr(self, "_plan", None) is not None else 0

    # ---- stepping the plan by hand (nfisam_nsf_train_plan_begin / enqueue / peek / stream / end) ----------------------
    def begin(self):
        """Start a hand-stepped run of the (graph) plan: chunks are enqueued with `enqueue`, looked at with `peek`."""
        self.prepare(True)
        _check(lib().nfisam_nsf_train_plan_begin(self._plan, _stream()), "nfisam_nsf_train_plan_begin")
        if getattr(self, "_plan_stream", None) is None:
            self._plan_stream = torch.cuda.ExternalStream(int(lib().nfisam_nsf_train_plan_stream(self._plan)), device=self.device)
            self._peek = (TrainState * self.nc)()

    def enqueue(self):
        """Append one chunk of iterations to the plan's stream (non-blocking)."""
        _check(lib().nfisam_nsf_train_plan_enqueue(self._plan), "nfisam_nsf_train_plan_enqueue")

    def peek(self):
        """-> (chunks closed since `begin`, [(step, stop, domain_err) per clique]) as of the last closed chunk; chunks = -1
        when a chunk closed while the mirror was being copied (look again)."""
        _check(lib().nfisam_nsf_train_plan_peek(self._plan, self._peek), "nfisam_nsf_train_plan_peek")
        seq = min(int(s.reserved[0]) for s in self._peek)
        return seq, [(int(s.step), int(s.stop), int(s.domain_err)) for s in self._peek]

    def feed(self, depth):
        """The library's feeder thread keeps `depth` chunks enqueued ahead of the last closed one (0: pause)."""
        _check(lib().nfisam_nsf_train_plan_feed(self._plan, int(depth)), "nfisam_nsf_train_plan_feed")

    def enqueued(self):
        return int(lib().nfisam_nsf_train_plan_enqueued(self._plan))

    def refill(self, c, x, kparams):
        """Slot c gets a NEW problem of the same shape: batch, fresh parameters, zeroed moments / workspace / loss record and
        -- last -- state, enqueued on the plan's stream behind the chunks already there (the slot's old clique must have
        stopped: nothing writes its buffers any more).  `x` / `kparams` (float32, contiguous, produced on the current stream)
        must stay alive until the copies have run -- keep a reference as long as the slot trains them."""
        if x.shape != self.xs[c].shape or kparams.numel() != self.kparams[c].numel() or x.dtype != torch.float32 or \
                kparams.dtype != torch.float32 or not x.is_contiguous() or not kparams.is_contiguous() or x.device != self.device:
            raise ValueError("refill needs a contiguous float32 batch and parameters of the slot's shape on the plan's device")
        _check(lib().nfisam_nsf_train_plan_refill(self._plan, int(c), C.c_void_p(x.data_ptr()), C.c_void_p(kparams.data_ptr()),
                                                  _stream()), "nfisam_nsf_train_plan_refill")

    def end(self):
        """The current stream continues behind everything enqueued on the plan."""
        _check(lib().nfisam_nsf_train_plan_end(self._plan, _stream()), "nfisam_nsf_train_plan_end")

    def reset(self, kparams=None):
        """Re-initialise Adam moments / state / loss record in place (pointers stay valid, so a
        prepared plan can be re-run)."""
        for c in range(self.nc):
            if kparams is not None:
                self.kparams[c].copy_(kparams[c])
            self.m[c].zero_(); self.v[c].zero_(); self.g[c].zero_(); self.iter_loss[c].zero_()
            if self.x_val is not None:
                self.val_loss[c].zero_()
        self.states.zero_()

    def close(self):
        if getattr(self, "_plan", None) is not None:
            lib().nfisam_nsf_train_plan_destroy(self._plan)
            self._plan = None
            self._plan_stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def state(self, c=0):
        s = self.states[c].cpu().numpy()
        return {"step": int(s[0]), "stop": int(s[1]), "have_avg": int(s[2]),
                "loss_avg": float(s[3:4].view(np.float32)[0]), "domain_err": int(s[4]), "slower_stop_iter": int(s[7])}


def posterior_walk(entries, total_dim, n, K, H, B, L, device, generator=None, Zt=None):
    """Sample a whole Bayes tree root -> leaves in one launch.

    entries: list (parents before children) of dicts with keys
        kparams, mean, std, circular (device tensors), D_model, obs (1-D numpy), sep_cols, front_cols (lists of
        column indices into the [n, total_dim] sample matrix).
    -> device tensor [n, total_dim] (float32) of posterior samples."""
    nc = len(entries)
    table = (PostClique * nc)()
    cols, obs = [], []
    max_D = 1
    for e, q in zip(entries, table):
        q.kparams = e["kparams"].data_ptr(); q.mean = e["mean"].data_ptr(); q.std = e["std"].data_ptr()
        q.circular = e["circular"].data_ptr()
        q.D_model = int(e["D_model"]); q.n_obs = len(e["obs"]); q.n_sep = len(e["sep_cols"])
        q.n_frontal = len(e["front_cols"])
        if q.n_obs + q.n_sep + q.n_frontal > q.D_model:
            raise ValueError("clique columns exceed its model dimension")
        q.obs_off = len(obs); obs.extend(float(v) for v in e["obs"])
        q.sep_off = len(cols); cols.extend(int(v) for v in e["sep_cols"])
        q.front_off = len(cols); cols.extend(int(v) for v in e["front_cols"])
        max_D = max(max_D, q.D_model)
    if sum(int(q.n_frontal) for q in table) > int(total_dim) or (cols and not 0 <= min(cols) <= max(cols) < int(total_dim)):
        raise ValueError("the cliques' frontal columns exceed the %d columns of the sample matrix (one latent row of Zt per "
                         "frontal column, consumed in walk order), or a column index is out of range" % total_dim)
    tbl = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(device)
    cols_t = torch.tensor(cols if cols else [0], dtype=torch.int32, device=device)
    obs_t = torch.tensor(obs if obs else [0.0], dtype=torch.float32, device=device)
    if Zt is None:
        Zt = torch.randn(total_dim, n, dtype=torch.float32, device=device, generator=generator)
    Zt = _dev(Zt, "Zt")
    if tuple(Zt.shape) != (total_dim, n):
        raise ValueError("Zt must be [total_dim, n] (column-major sample layout)")
    St = torch.zeros(total_dim, n, dtype=torch.float32, device=device)
    _check(lib().nfisam_nsf_posterior_walk(C.c_void_p(tbl.data_ptr()), nc, _ptr(cols_t), _ptr(obs_t), max_D, int(K),
                                           int(H), C.c_float(B), int(L), int(n), _ptr(Zt), _ptr(St), _stream()),
           "nfisam_nsf_posterior_walk")
    return St.t().contiguous()


class SimOp(C.Structure):
    """`nfisam_sim_op` (include/nfisam_hip.h)."""
    _fields_ = [("code", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("cand", C.c_int32 * 4),
                ("k", C.c_int32), ("p", C.c_float * 9), ("src", C.c_uint64)]


SIM_MAX_OPS = 40
SIM_COPY, SIM_PRIOR_SE2, SIM_REL_FWD, SIM_REL_BWD, SIM_REL_OBS, SIM_RING, SIM_RANGE_OBS, SIM_ADA_OBS, SIM_NH_RING, \
    SIM_NH_OBS, SIM_PRIOR_R2, SIM_PRIOR_R2_RING, SIM_REL_R2_FWD, SIM_REL_R2_BWD, SIM_REL_R2_OBS = range(1, 16)
assert C.sizeof(SimOp) == 80


def simulate_clique(ops, n, D_out, D_total, seed, device):
    """Run a compiled simulation schedule (list of SimOp) -> device tensor [n, D_out] float32."""
    arr = (SimOp * len(ops))(*ops)
    out = torch.empty(int(n), int(D_out), dtype=torch.float32, device=device)
    _check(lib().nfisam_simulate_clique(arr, len(ops), int(n), int(D_out), int(D_total), C.c_uint64(int(seed)), _ptr(out),
                                        _stream()), "nfisam_simulate_clique")
    return out


def normalize_columns(x, circular=None):
    """NFiSAM.normalize_training_samples on the device: x [n, D] float32 (cuda) -> (x_normalised, mean[D], std[D])."""
    x = _dev(x, "x")
    n, D = x.shape
    circ = None
    if circular is not None:
        circ, = upload(np.asarray(circular, dtype=np.uint8), device=x.device)
    out = torch.empty_like(x)
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    std = torch.empty(D, dtype=torch.float32, device=x.device)
    _check(lib().nfisam_normalize_columns(_ptr(x), int(n), int(D), _ptr(circ) if circ is not None else None, _ptr(out),
                                          _ptr(mean), _ptr(std), _stream()), "nfisam_normalize_columns")
    return out, mean, std


POST_DTYPE = np.dtype([("kparams", np.uint64), ("mean", np.uint64), ("std", np.uint64), ("circular", np.uint64),
                       ("D_model", np.int32), ("n_obs", np.int32), ("n_sep", np.int32), ("n_frontal", np.int32),
                       ("obs_off", np.int32), ("sep_off", np.int32), ("front_off", np.int32), ("reserved", np.int32)])
assert POST_DTYPE.itemsize == C.sizeof(PostClique)


def posterior_walk_raw(table: np.ndarray, cols: np.ndarray, obs: np.ndarray, total_dim, n, max_D, K, H, B, L, device,
                       Zt=None):
    """`posterior_walk` with the clique table already assembled as a numpy array of POST_DTYPE
    (callers that walk large trees every update cache the per-clique pointers)."""
    if int(table["n_frontal"].sum()) > int(total_dim) or (cols.size and not 0 <= int(cols.min()) <= int(cols.max()) < int(total_dim)):
        raise ValueError("the cliques' frontal columns exceed the %d columns of the sample matrix, or a column index is out of range"
                         % total_dim)
    if Zt is not None and tuple(Zt.shape) != (int(total_dim), int(n)):
        raise ValueError("Zt must be [total_dim, n] (column-major sample layout)")
    tbl, cols_t, obs_t = upload(table.view(np.uint8).reshape(-1), np.asarray(cols if cols.size else np.zeros(1), dtype=np.int32),
                                np.asarray(obs if obs.size else np.zeros(1), dtype=np.float32), device=device)
    if Zt is None:
        Zt = torch.randn(total_dim, n, dtype=torch.float32, device=device)
    St = torch.zeros(total_dim, n, dtype=torch.float32, device=device)
    _check(lib().nfisam_nsf_posterior_walk(C.c_void_p(tbl.data_ptr()), int(table.shape[0]), _ptr(cols_t), _ptr(obs_t),
                                           int(max_D), int(K), int(H), C.c_float(B), int(L), int(n), _ptr(Zt), _ptr(St),
                                           _stream()), "nfisam_nsf_posterior_walk")
    return St.t().contiguous()


def check_posterior_table(table: np.ndarray, cols, obs, total_dim: int, max_D, K, H, B, L, latent=False):
    """ValueError for a clique table the log-density kernel must not see -> (cols int32, obs float32), flattened."""
    if not isinstance(table, np.ndarray) or table.dtype != POST_DTYPE or table.ndim != 1:
        raise ValueError("table must be a 1-D numpy array of POST_DTYPE")
    cols = np.asarray(cols, dtype=np.int32).reshape(-1)
    obs = np.asarray(obs, dtype=np.float32).reshape(-1)
    if not supported(K, H):
        raise ValueError("num_knots=%r, hidden_dim=%r: no kernels for this (K, H)" % (K, H))
    if int(L) < 1 or not float(B) > 0 or int(max_D) < 1:
        raise ValueError("L >= 1, B > 0 and max_D >= 1 are required")
    if int(table.shape[0]):
        n_obs, n_sep, n_fr = (table[f].astype(np.int64) for f in ("n_obs", "n_sep", "n_frontal"))
        Dm = table["D_model"].astype(np.int64)
        if (min(n_obs.min(), n_sep.min(), n_fr.min()) < 0 or np.any(n_obs + n_sep + n_fr > Dm) or Dm.max() > int(max_D)
                or Dm.min() < 1):
            raise ValueError("a clique's columns exceed its model dimension, or a model dimension exceeds max_D")
        if (np.any(table["obs_off"] < 0) or np.any(table["sep_off"] < 0) or np.any(table["front_off"] < 0)
                or np.any(table["obs_off"] + n_obs > obs.size) or np.any(table["sep_off"] + n_sep > cols.size)
                or np.any(table["front_off"] + n_fr > cols.size)):
            raise ValueError("a clique's offsets run past `obs` / `cols`")
        if cols.size and not 0 <= int(cols.min()) <= int(cols.max()) < total_dim:
            raise ValueError("a column index is out of range of the %d columns of S" % total_dim)
        if latent and int(n_fr.sum()) > total_dim:
            raise ValueError("the cliques' frontal columns exceed the %d latent rows" % total_dim)
    return cols, obs


def posterior_log_density(table: np.ndarray, cols: np.ndarray, obs: np.ndarray, S, max_D, K, H, B, L, device,
                          per_clique=False, latent=False):
    """Joint log-density of the tree's posterior at the n rows of S (nfisam_nsf_posterior_log_density): the clique table
    of `posterior_walk_raw` (numpy POST_DTYPE, parents first), S [n, total_dim] as the walk returns it (tensor or numpy).
    Launched on the current stream.  -> log_q [n] (device tensor); with per_clique or latent: (log_q, per [n_cliques, n] or
    None, latent [total_dim, n] or None) -- `latent` holds z of every frontal column at the row of Zt the walk reads that
    column's draw from (rows of no frontal column are zero)."""
    cols, obs = check_posterior_table(table, cols, obs, _points_width(S), max_D, K, H, B, L, latent)
    return posterior_log_density_t(table, cols, obs, _columns(S, device), max_D, K, H, B, L, device, per_clique=per_clique,
                                   latent=latent, checked=True)


def posterior_log_density_t(table: np.ndarray, cols: np.ndarray, obs: np.ndarray, St, max_D, K, H, B, L, device,
                            per_clique=False, latent=False, checked=False):
    """`posterior_log_density` on the COLUMN-major matrix St [total_dim, n] (contiguous float32 device tensor): what the tree
    walk wrote, scored in place.  `checked` skips the table check (the caller has made it)."""
    total_dim, n = _points_shape_t(St)
    if not checked:
        cols, obs = check_posterior_table(table, cols, obs, total_dim, max_D, K, H, B, L, latent)
    nc = int(table.shape[0])
    log_q = torch.empty(n, dtype=torch.float32, device=device)
    # the per-clique terms are the first pass's output; they come from torch's allocator even when the caller does not want
    # them (the C entry would otherwise take a scratch buffer from HIP's own stream-ordered pool)
    per = torch.empty(nc, n, dtype=torch.float32, device=device)
    lat = torch.zeros(total_dim, n, dtype=torch.float32, device=device) if latent else None
    if nc == 0 or n == 0:
        log_q.zero_()                                       # the empty tree / no points: nothing to launch
    else:
        tbl, cols_t, obs_t = upload(table.view(np.uint8).reshape(-1), cols if cols.size else np.zeros(1, dtype=np.int32),
                                    obs if obs.size else np.zeros(1, dtype=np.float32), device=device)
        _check(lib().nfisam_nsf_posterior_log_density(C.c_void_p(tbl.data_ptr()), nc, _ptr(cols_t), _ptr(obs_t), int(max_D),
                                                      int(K), int(H), C.c_float(B), int(L), n, _ptr(St), _ptr(log_q), _ptr(per),
                                                      _ptr(lat), _stream()), "nfisam_nsf_posterior_log_density")
    if per_clique or latent:
        return log_q, (per if per_clique else None), lat
    return log_q


# ---- the factor graph's joint log-density (nfisam_factor_graph_log_density) ------------------------------------------------------
FACTOR_DTYPE = np.dtype([("code", np.int32), ("a", np.int32), ("b", np.int32), ("k", np.int32), ("cand", np.int32, (4,)),
                         ("p", np.float64, (16,))])
assert FACTOR_DTYPE.itemsize == C.sizeof(FactorTerm)
# NFISAM_FAC_* of include/nfisam_hip.h; _FAC_ROWS: code -> (rows of St read at `a`, at `b` or 0), as csrc/factor_model.h has them
FAC_CODES = {"PRIOR_SE2": 1, "REL_SE2": 2, "RANGE": 3, "RANGE_MIX": 4, "PRIOR_R2": 5, "PRIOR_R2_RANGE": 6, "REL_R2": 7}
_FAC_ROWS = {1: (3, 0), 2: (3, 3), 3: (2, 2), 4: (2, 0), 5: (2, 0), 6: (2, 0), 7: (2, 2)}


def pack_factor_terms(factors, row_of) -> np.ndarray:
    """The device table of `factors` (numpy FACTOR_DTYPE, one record per factor, in order): every factor's
    `density_record()` with its variables replaced by their first rows `row_of[variable]` of the sample matrix.
    NotImplementedError names the class of a factor without a device code."""
    t = np.zeros(len(factors), dtype=FACTOR_DTYPE)
    for i, f in enumerate(factors):
        rec = getattr(f, "density_record", None)
        if rec is None:
            raise NotImplementedError("factor class %s has no device code for the joint log-density" % f.__class__.__name__)
        r = rec()
        cand = [row_of[v] for v in r["cand"]]
        if len(cand) > 4 or len(r["p"]) > 16:
            raise NotImplementedError("%s: %d components, the device table holds at most 4" % (f.__class__.__name__, len(cand)))
        t["code"][i] = FAC_CODES[r["code"]]
        t["a"][i] = row_of[r["a"]]
        t["b"][i] = row_of[r["b"]] if r["b"] is not None else 0
        t["k"][i] = len(cand)
        t["cand"][i, :len(cand)] = cand
        t["p"][i, :len(r["p"])] = r["p"]
    return t


def check_factor_terms(terms: np.ndarray, total_dim: int) -> None:
    """ValueError for a table the kernel must not see: an unknown code, k outside 1..4, a row outside [0, total_dim)."""
    if not isinstance(terms, np.ndarray) or terms.dtype != FACTOR_DTYPE or terms.ndim != 1:
        raise ValueError("terms must be a 1-D numpy array of FACTOR_DTYPE")
    if terms.size == 0:
        return
    code = terms["code"]
    known = np.isin(code, list(_FAC_ROWS))
    if not np.all(known):
        raise ValueError("unknown factor code %d" % int(code[~known][0]))
    mix = code == FAC_CODES["RANGE_MIX"]
    if np.any((terms["k"][mix] < 1) | (terms["k"][mix] > 4)):
        raise ValueError("a mixture must have 1..4 components")
    rows_a = np.array([_FAC_ROWS[int(c)][0] for c in code])
    rows_b = np.array([_FAC_ROWS[int(c)][1] for c in code])
    a, b = terms["a"].astype(np.int64), terms["b"].astype(np.int64)
    bad = (a < 0) | (a + rows_a > total_dim) | ((rows_b > 0) & ((b < 0) | (b + rows_b > total_dim)))
    used = np.arange(4)[None, :] < terms["k"][:, None]
    cand = terms["cand"].astype(np.int64)
    bad |= mix & np.any(used & ((cand < 0) | (cand + 2 > total_dim)), axis=1)
    if np.any(bad):
        raise ValueError("factor %d: a variable row is out of range of the %d columns of S" % (int(np.argmax(bad)), total_dim))


def factor_graph_log_density(terms: np.ndarray, S, device, per_factor=False, terms_dev=None):
    """log p(X, Z) = the sum of the factors' log densities at the n rows of S (nfisam_factor_graph_log_density): `terms` the
    numpy FACTOR_DTYPE table (`pack_factor_terms`), S [n, total_dim] in the walk's column layout (tensor or numpy; float32
    points, the arithmetic is float64).  Launched on the current stream.  `terms_dev`: an uploaded copy of `terms` to reuse
    (uint8 device tensor, kept by callers that score every update).
    -> log_p [n] float64 device tensor; with per_factor: (log_p, per [n_terms, n] float64)."""
    check_factor_terms(terms, _points_width(S))
    return factor_graph_log_density_t(terms, _columns(S, device), device, per_factor=per_factor, terms_dev=terms_dev, checked=True)


def factor_graph_log_density_t(terms: np.ndarray, St, device, per_factor=False, terms_dev=None, checked=False):
    """`factor_graph_log_density` on the COLUMN-major matrix St [total_dim, n] (contiguous float32 device tensor): what the
    tree walk wrote, scored in place."""
    total_dim, n = _points_shape_t(St)
    if not checked:
        check_factor_terms(terms, total_dim)
    nt = int(terms.shape[0])
    log_p = torch.empty(n, dtype=torch.float64, device=device)
    # the per-factor terms are the first pass's output; they come from torch's allocator even when the caller does not want
    # them (the C entry would otherwise take a scratch buffer from HIP's own stream-ordered pool)
    per = torch.empty(nt, n, dtype=torch.float64, device=device)
    if nt == 0 or n == 0:
        log_p.zero_()                                       # the empty graph / no points: nothing to launch
    else:
        dev = _factor_tables(device, terms, terms_dev)
        _check(lib().nfisam_factor_graph_log_density(_ptr(dev["terms"]), nt, _ptr(St), total_dim, n, _ptr(log_p), _ptr(per),
                                                     _stream()), "nfisam_factor_graph_log_density")
    return (log_p, per) if per_factor else log_p


# ---- the front of the sample bindings: what every evaluator over the walk's sample matrix checks and stages ---------------------
# Every binding below comes as NAME(X [n, cols], ..., device), which makes every check on a row-major tensor or array before
# the device is touched and hands the transposed copy on, and as NAME_t(Xt [rows, n], ..., checked=True), which works on the
# column-major device matrix in place.  A new evaluator is written from these helpers (csrc/sample_common.h on the device
# side): the two fronts (`_two_set_front` / `_two_set_upload` where two sample sets meet), the block-table checks, `_f64` for
# the weights, which go the plain way, and `_upload_named` for everything small -- ONE `upload` per call for whatever is on the
# host, every result taken by name, whatever form it came in.
def _row_major_front(what, device, **mats):
    """The head of the row-major binding `what`: -> the device (default: the first matrix's own, or "cuda").  RuntimeError
    unless that is a ROCm device, ValueError unless every matrix is a 2-D tensor or array.  Nothing is copied yet: `_columns`
    does that once the caller's tables have passed their checks."""
    first = next(iter(mats.values()))
    if device is None:
        device = first.device if torch.is_tensor(first) else "cuda"
    if torch.device(device).type != "cuda":
        raise RuntimeError("%s needs a ROCm device (no CPU path exists)" % what)
    if not all((torch.is_tensor(A) or isinstance(A, np.ndarray)) and A.ndim == 2 for A in mats.values()):
        raise ValueError("%s must be %s" % (" and ".join(mats), "a [rows, cols] tensor or array" if len(mats) == 1 else
                                            "[rows, cols] tensors or arrays"))
    return device


def _columns(A, device):
    """A [n, cols] (tensor or numpy) -> the column-major float32 matrix [cols, n] on `device`."""
    if torch.is_tensor(A):
        return A.to(device=device, dtype=torch.float32).t().contiguous()
    return torch.from_numpy(np.ascontiguousarray(A.T, dtype=np.float32)).to(device)


def _column_major_front(name, t):
    """The head of a column-major binding: `t` must be a contiguous float32 [rows, points] tensor on a ROCm device
    -> (rows, points)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on a ROCm device (no CPU path exists)" % name)
    if t.ndim != 2 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float32 [rows, points] tensor" % name)
    return int(t.shape[0]), int(t.shape[1])


def _two_set_front(names, At, Bt, same=False):
    """The head of a column-major binding over two sets, `names` their arguments' names: both pass `_column_major_front` and
    lie on one device; with `same`, Bt None is At -> (Bt, a_rows, m, b_rows, n)."""
    a_rows, m = _column_major_front(names[0], At)
    if same and Bt is None:
        Bt = At
    b_rows, n = _column_major_front(names[1], Bt)
    if At.device != Bt.device:
        raise ValueError("%s and %s must be on the same device" % tuple(names))
    return Bt, a_rows, m, b_rows, n


def _two_set_upload(device, blocks, names, acols, bcols, **per_entry):
    """What such a binding stages, in ONE `upload`: the contiguous table `blocks`, the two column lists as int32 under `names`
    and the per-entry arrays -> ({name: tensor on `device`}, the number of entries)."""
    ac, bc = np.asarray(acols, dtype=np.int32), np.asarray(bcols, dtype=np.int32)
    return _upload_named(device, blocks=_table_bytes(blocks), **{names[0]: ac, names[1]: bc}, **per_entry), int(ac.size)


def _f64(a, device):
    """None, a tensor or anything numpy takes -> None or a contiguous float64 tensor on `device` (the plain way: one `.to`)."""
    if a is None:
        return None
    if torch.is_tensor(a):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _entry_f64(a):
    """An optional float64 per-entry array in the form `_upload_named` takes: None, a device tensor cast to float64 (it stays
    where it is), or -- a list, numpy, a CPU tensor -- the float64 numpy array to stage."""
    if a is None:
        return None
    if torch.is_tensor(a) and a.is_cuda:
        return a.to(dtype=torch.float64)
    return np.ascontiguousarray(a, dtype=np.float64)


def _flags(a):
    """Optional per-entry flags -> None or the uint8 numpy array the kernels read."""
    return None if a is None else np.asarray(a).astype(np.uint8)


def _table_bytes(blocks):
    return blocks.view(np.uint8).reshape(-1)


# the factor evaluators' front: a bad S or table is a ValueError before the device matters, then `_columns(S, device)` copies
def _points_width(S):
    if not (torch.is_tensor(S) or isinstance(S, np.ndarray)) or S.ndim != 2:
        raise ValueError("S must be a [n, total_dim] tensor or array")
    return int(S.shape[1])


def _points_shape_t(St):
    if not torch.is_tensor(St) or St.ndim != 2 or St.dtype != torch.float32 or not St.is_contiguous():
        raise ValueError("St must be a contiguous float32 [total_dim, n] tensor")
    return int(St.shape[0]), int(St.shape[1])


def _factor_tables(device, terms, terms_dev, **lists):
    """-> {"terms": the table's device copy (`terms_dev` reused, else `terms` uploaded), **`lists`}: ONE staged copy for the rest."""
    return _upload_named(device, terms=terms_dev if terms_dev is not None else _table_bytes(np.ascontiguousarray(terms)), **lists)


def _upload_named(device, **arrays):
    """`upload` by name: ONE staged copy for the numpy arrays among `arrays` (none at all if there is none); a value that is
    a tensor already is not staged but brought to `device`, contiguous; None stays None.
    -> {name: tensor on `device`, None for an absent array}: what a name maps to never depends on the form of another."""
    host = {k: a for k, a in arrays.items() if a is not None and not torch.is_tensor(a)}
    out = {k: a.to(device).contiguous() if torch.is_tensor(a) else None for k, a in arrays.items()}
    if host:
        out.update(zip(host, upload(*host.values(), device=device)))
    return out


def _check_table_layout(blocks, dtype, dtype_name, cols, per_entry, max_d=None):
    """What the block-table checks share, in this order (a checker goes on with what is its own, then `_check_bandwidths`
    and `_check_rows`): the table's dtype, the column lists `cols` ({name: (list, rows of
    its matrix)}: 1-D, one length >= 1), the optional per-entry arrays `per_entry` ({name: array or None}: that length),
    1..65535 blocks, widths in 1..max_d (if given), entries inside [0, n_entries).  -> (col_off, d) as int64."""
    if not isinstance(blocks, np.ndarray) or blocks.dtype != dtype or blocks.ndim != 1:
        raise ValueError("blocks must be a 1-D numpy array of %s" % dtype_name)
    lists = [np.asarray(c) for c, _ in cols.values()]
    ne, single = int(lists[0].size), len(lists) == 1
    if ne < 1 or any(c.ndim != 1 or c.size != ne for c in lists):
        raise ValueError("cols must be a 1-D list of at least one row" if single else
                         "%s must be 1-D lists of the same length >= 1" % " and ".join(cols))
    for name, a in per_entry.items():
        if a is not None and (tuple(a.shape) if torch.is_tensor(a) else np.shape(a)) != (ne,):
            raise ValueError("%s must have one %s per entry (%d)" % (name, "flag" if name == "circular" else "value", ne))
    if not 1 <= blocks.size <= 65535:
        raise ValueError("1..65535 blocks are supported, got %d" % blocks.size)
    off, d = blocks["col_off"].astype(np.int64), blocks["d"].astype(np.int64)
    if max_d is not None and np.any((d < 1) | (d > max_d)):
        b = int(np.argmax((d < 1) | (d > max_d)))
        raise ValueError("block %d: width %d is outside 1..%d" % (b, int(d[b]), max_d))
    bad = (d < 1) | (off < 0) | (off + d > ne)
    if np.any(bad):
        b = int(np.argmax(bad))
        raise ValueError("block %d: entries %d..%d leave the %d entries of the column list%s"
                         % (b, int(off[b]), int((off + d)[b]), ne, "" if single else "s (d >= 1 is required)"))
    return off, d


def _check_bandwidths(blocks):
    ok = np.isfinite(blocks["inv_two_sigma2"]) & (blocks["inv_two_sigma2"] > 0)
    if not np.all(ok):
        raise ValueError("block %d: inv_two_sigma2 must be positive and finite" % int(np.argmin(ok)))


def _check_finite(name, a):
    """ValueError unless the optional host array `a` holds finite values alone."""
    if a is not None and not np.all(np.isfinite(np.asarray(a, dtype=np.float64))):
        raise ValueError("%s must be finite" % name)


def _consecutive(dims, dtype):
    """-> (dims as int64 [n_blocks], the zeroed table of `dtype` with d = dims and col_off = the blocks one after another)."""
    dims = np.asarray(dims, dtype=np.int64).reshape(-1)
    t = np.zeros(dims.size, dtype=dtype)
    t["d"], t["col_off"] = dims, np.cumsum(dims) - dims
    return dims, t


def _check_rows(cols):
    """Every row of the column lists `cols` ({name: (list, rows of its matrix)}) inside its matrix."""
    for name, (c, rows) in cols.items():
        c = np.asarray(c)
        if not 0 <= int(c.min()) <= int(c.max()) < int(rows):
            raise ValueError("%s: a row is out of range of the %d rows of %s matrix"
                             % (name, int(rows), "the" if len(cols) == 1 else "its"))


def _check_disjoint(off, d, why):
    """No two blocks of (col_off, d) share an entry: for results that are stored by entry (`why` says which)."""
    order = np.argsort(off, kind="stable")
    clash = (off[order][1:] < (off + d)[order][:-1])
    if np.any(clash):
        raise ValueError("blocks %d and %d share an entry: %s"
                         % (int(order[:-1][np.argmax(clash)]), int(order[1:][np.argmax(clash)]), why))


def _score_front(name, Gt, Xt):
    """The head of a binding that reads a score matrix next to the points `Xt`: `Gt` must be a contiguous float64
    [rows, points] tensor on Xt's ROCm device (its shape is the caller's check)."""
    if not torch.is_tensor(Gt) or not Gt.is_cuda:
        raise RuntimeError("%s must be a tensor on a ROCm device (no CPU path exists)" % name)
    if Gt.ndim != 2 or Gt.dtype != torch.float64 or not Gt.is_contiguous():
        raise ValueError("%s must be a contiguous float64 [rows, points] tensor" % name)
    if Gt.device != Xt.device:
        raise ValueError("Xt and %s must be on the same device" % name)


# ---- two-sample MMD: the kernel sums of many column blocks in one launch (nfisam_sample_mmd) ------------------------------------
MMD_BLOCK_DTYPE = np.dtype([("col_off", np.int32), ("d", np.int32), ("inv_two_sigma2", np.float64)])
assert MMD_BLOCK_DTYPE.itemsize == C.sizeof(MmdBlock)


def pack_mmd_blocks(dims, sigmas) -> np.ndarray:
    """The block table (numpy MMD_BLOCK_DTYPE) of consecutive blocks of `dims` entries with kernel bandwidths `sigmas`."""
    dims, t = _consecutive(dims, MMD_BLOCK_DTYPE)
    t["inv_two_sigma2"] = 1.0 / (2.0 * np.asarray(sigmas, dtype=np.float64).reshape(-1) ** 2)
    return t


def check_mmd_blocks(blocks: np.ndarray, xcols, ycols, x_rows: int, y_rows: int, scale=None, wrap=None) -> None:
    """ValueError for tables the kernel must not see: no block or more than 65535, d < 1, a bandwidth term that is not positive
    and finite, entries outside [0, n_entries), a row outside [0, x_rows) / [0, y_rows), per-entry arrays of another length."""
    cols = {"xcols": (xcols, x_rows), "ycols": (ycols, y_rows)}
    _check_table_layout(blocks, MMD_BLOCK_DTYPE, "MMD_BLOCK_DTYPE", cols, dict(scale=scale, wrap=wrap))
    _check_bandwidths(blocks)
    _check_rows(cols)
    _check_finite("scale", scale)


def mmd_sums(X, Y, blocks: np.ndarray, xcols, ycols, scale=None, wrap=None, device=None):
    """The kernel sums {Sxx, Syy, Sxy} of every block of `blocks` between the sample sets X [m, x_cols] and Y [n, y_cols]
    (tensor or numpy; float32 points, float64 arithmetic): nfisam_sample_mmd, one launch for all blocks on the current
    stream.  `blocks`: numpy MMD_BLOCK_DTYPE (`pack_mmd_blocks`); entry e of a block pairs column xcols[e] of X with column
    ycols[e] of Y; scale [n_entries] multiplies an entry's differences, wrap [n_entries] marks angles (differences brought
    into [-pi, pi)).  -> [n_blocks, 3] float64 device tensor."""
    device = _row_major_front("mmd_sums", device, X=X, Y=Y)
    check_mmd_blocks(blocks, xcols, ycols, int(X.shape[1]), int(Y.shape[1]), scale, wrap)
    return mmd_sums_t(_columns(X, device), _columns(Y, device), blocks, xcols, ycols, scale, wrap, checked=True)


def mmd_sums_t(Xt, Yt, blocks: np.ndarray, xcols, ycols, scale=None, wrap=None, checked=False):
    """`mmd_sums` on the COLUMN-major matrices Xt [x_rows, m], Yt [y_rows, n] (contiguous float32 device tensors, used in
    place): what the tree walk wrote."""
    Yt, x_rows, m, y_rows, n = _two_set_front(("Xt", "Yt"), Xt, Yt)
    device = Xt.device
    if m < 1 or n < 1:
        raise ValueError("both sample sets need at least one point")
    if not checked:
        check_mmd_blocks(blocks, xcols, ycols, x_rows, y_rows, scale, wrap)
    nb = int(blocks.shape[0])
    blocks = np.ascontiguousarray(blocks)
    with torch.cuda.device(device):
        dev, ne = _two_set_upload(device, blocks, ("xcols", "ycols"), xcols, ycols, scale=_entry_f64(scale), wrap=_flags(wrap))
        count = int(lib().nfisam_sample_mmd_scratch_count(m, n, nb))
        if count < 1:
            raise ValueError("mmd_sums: %d x %d points in %d blocks exceed the grid" % (m, n, nb))
        # the per-tile partials come from torch's allocator, like the per-factor rows of factor_graph_log_density_t
        scratch = torch.empty(count, dtype=torch.float64, device=device)
        sums = torch.empty(nb, 3, dtype=torch.float64, device=device)
        _check(lib().nfisam_sample_mmd(_ptr(Xt), x_rows, m, _ptr(Yt), y_rows, n, blocks.ctypes.data_as(C.c_void_p),
                                       _ptr(dev["blocks"]), nb, _ptr(dev["xcols"]), _ptr(dev["ycols"]), ne,
                                       _ptr(dev["scale"]), _ptr(dev["wrap"]), _ptr(sums), _ptr(scratch), _stream()),
               "nfisam_sample_mmd")
    return sums


# ---- sliced Wasserstein: every (block, direction) slice of two sample sets in one launch (nfisam_sample_sliced_transport) ------
TRANSPORT_BLOCK_DTYPE = np.dtype([("col_off", np.int32), ("d", np.int32), ("n_dirs", np.int32), ("reserved", np.int32),
                                  ("dir_off", np.int64), ("out_off", np.int64)])
assert TRANSPORT_BLOCK_DTYPE.itemsize == C.sizeof(TransportBlock)
TRANSPORT_MAX_N = 8192                   # NFISAM_TRANSPORT_MAX_N: points per set (two lists of float64 keys in LDS)
TRANSPORT_KINDS = (0, 1, 2)              # what an entry contributes: the value, its cosine, its sine


def pack_transport_blocks(dims, n_dirs) -> np.ndarray:
    """The block table (numpy TRANSPORT_BLOCK_DTYPE) of consecutive blocks of `dims` entries with `n_dirs` directions each
    (one count, or one per block): block b's directions are the doubles dir_off .. dir_off + n_dirs * d of the direction
    array, [n_dirs, d] row-major, and its slices out_off .. out_off + n_dirs of the result, both in table order."""
    dims, t = _consecutive(dims, TRANSPORT_BLOCK_DTYPE)
    nd = np.broadcast_to(np.asarray(n_dirs, dtype=np.int64).reshape(-1), dims.shape) if np.size(n_dirs) == 1 else \
        np.asarray(n_dirs, dtype=np.int64).reshape(-1)
    if nd.shape != dims.shape:
        raise ValueError("n_dirs: one count, or one per block (%d), got %d" % (dims.size, nd.size))
    t["n_dirs"] = nd
    t["dir_off"] = np.cumsum(dims * nd) - dims * nd
    t["out_off"] = np.cumsum(nd) - nd
    return t


def check_transport_blocks(blocks: np.ndarray, xcols, ycols, x_rows: int, y_rows: int, dirs, kind=None, scale=None) -> int:
    """ValueError for tables the kernel must not see: what `_check_table_layout` and `_check_rows` refuse (no block or more
    than 65535, d < 1, entries outside [0, n_entries), a row outside its matrix, per-entry arrays of another length), a
    direction count outside 1..65535, a kind outside 0..2, directions that are not a 1-D float array of exactly the doubles
    the table names, slices that start below 0 or that two blocks share, a non-finite direction or scale.
    -> the number of slices (the length of the result)."""
    cols = {"xcols": (xcols, x_rows), "ycols": (ycols, y_rows)}
    off, d = _check_table_layout(blocks, TRANSPORT_BLOCK_DTYPE, "TRANSPORT_BLOCK_DTYPE", cols, dict(kind=kind, scale=scale))
    _check_rows(cols)
    nd, doff, ooff = (blocks[k].astype(np.int64) for k in ("n_dirs", "dir_off", "out_off"))
    if np.any((nd < 1) | (nd > 65535)):
        b = int(np.argmax((nd < 1) | (nd > 65535)))
        raise ValueError("block %d: n_dirs = %d is outside 1..65535" % (b, int(nd[b])))
    if kind is not None and not np.all(np.isin(np.asarray(kind), TRANSPORT_KINDS)):
        raise ValueError("kind must be 0 (the value), 1 (its cosine) or 2 (its sine)")
    if torch.is_tensor(dirs) or np.ndim(dirs) != 1 or np.asarray(dirs).dtype.kind != "f":
        raise ValueError("dirs must be a 1-D float array (numpy): every block's [n_dirs, d] directions, flattened")
    dirs = np.asarray(dirs, dtype=np.float64)
    if np.any(doff < 0) or int((doff + nd * d).max()) != dirs.size:
        raise ValueError("dirs has %d values, the table names %d (block b: dir_off .. dir_off + n_dirs * d, dir_off >= 0)"
                         % (dirs.size, int((doff + nd * d).max())))
    if np.any(ooff < 0):
        raise ValueError("block %d: out_off must be >= 0" % int(np.argmax(ooff < 0)))
    _check_disjoint(ooff, nd, "every slice is stored once")
    _check_finite("dirs", dirs)
    _check_finite("scale", scale)
    return int((ooff + nd).max())


def _check_transport_sizes(m, n, p):
    if p not in (1, 2):
        raise ValueError("p must be 1 or 2, got %r" % (p,))
    if m < 1 or n < 1:
        raise ValueError("both sample sets need at least one point")
    if m > TRANSPORT_MAX_N or n > TRANSPORT_MAX_N:
        raise ValueError("sliced_transport sorts at most %d points per set in LDS, got %d and %d" % (TRANSPORT_MAX_N, m, n))


def sliced_transport(X, Y, blocks: np.ndarray, xcols, ycols, dirs, p=2, kind=None, scale=None, device=None):
    """W_p^p of the sample sets X [m, x_cols] and Y [n, y_cols] (tensor or numpy; float32 points, float64 arithmetic)
    projected on every direction of every block of `blocks`: nfisam_sample_sliced_transport, one launch on the current
    stream.  `blocks`: numpy TRANSPORT_BLOCK_DTYPE (`pack_transport_blocks`); entry e of a block pairs column xcols[e] of X
    with column ycols[e] of Y and contributes dir[e] * scale[e] * f(value) to a point's key, f by kind[e]: 0 the value, 1 its
    cosine, 2 its sine (a heading enters as two entries, cos and sin); dirs: the blocks' [n_dirs, d] directions, flattened
    (float64 numpy); p: 1 or 2.  At most TRANSPORT_MAX_N points per set.  -> [slices] float64 device tensor, block b's at
    out_off .. out_off + n_dirs; `Statistics.wasserstein_from_slices` forms the distances."""
    device = _row_major_front("sliced_transport", device, X=X, Y=Y)
    _check_transport_sizes(int(X.shape[0]), int(Y.shape[0]), p)
    check_transport_blocks(blocks, xcols, ycols, int(X.shape[1]), int(Y.shape[1]), dirs, kind, scale)
    return sliced_transport_t(_columns(X, device), _columns(Y, device), blocks, xcols, ycols, dirs, p, kind, scale, checked=True)


def sliced_transport_t(Xt, Yt, blocks: np.ndarray, xcols, ycols, dirs, p=2, kind=None, scale=None, checked=False):
    """`sliced_transport` on the COLUMN-major matrices Xt [x_rows, m], Yt [y_rows, n] (contiguous float32 device tensors, used
    in place): what the tree walk wrote."""
    Yt, x_rows, m, y_rows, n = _two_set_front(("Xt", "Yt"), Xt, Yt)
    device = Xt.device
    _check_transport_sizes(m, n, p)
    if not checked:
        check_transport_blocks(blocks, xcols, ycols, x_rows, y_rows, dirs, kind, scale)
    nb = int(blocks.shape[0])
    blocks = np.ascontiguousarray(blocks)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    n_out = int((blocks["out_off"].astype(np.int64) + blocks["n_dirs"]).max())
    with torch.cuda.device(device):
        dev, ne = _two_set_upload(device, blocks, ("xcols", "ycols"), xcols, ycols, kind=_flags(kind), scale=_entry_f64(scale),
                                  dirs=dirs)
        out = torch.full((n_out,), float("nan"), dtype=torch.float64, device=device)
        _check(lib().nfisam_sample_sliced_transport(_ptr(Xt), x_rows, m, _ptr(Yt), y_rows, n, blocks.ctypes.data_as(C.c_void_p),
                                                    _ptr(dev["blocks"]), nb, _ptr(dev["xcols"]), _ptr(dev["ycols"]),
                                                    _ptr(dev["kind"]), _ptr(dev["scale"]), ne, _ptr(dev["dirs"]),
                                                    C.c_longlong(int(dirs.size)), int(p), _ptr(out), C.c_longlong(n_out),
                                                    _stream()), "nfisam_sample_sliced_transport")
    return out


# ---- the MMD permutation test: the kernel sums under many relabellings of the pooled set (nfisam_sample_mmd_perm) -------------
MMD_PERM_MAX = 16384                     # NFISAM_MMD_PERM_MAX: permutations per launch
MMD_PERM_CHUNK = 256                     # the permutations one group of the kernel carries: calls are split at its multiples
MMD_PERM_SCRATCH_BYTES = 256 << 20       # a call's strip partials stay below this where 256 permutations a launch allow it


def pack_perm_labels(L) -> np.ndarray:
    """bool [P, m + n] (row p: which pooled points count as the first set under permutation p) -> uint64 [m + n, W],
    W = (P + 63) // 64: bit p & 63 of word [q][p >> 6], what nfisam_sample_mmd_perm reads."""
    L = np.asarray(L)
    if L.ndim != 2 or L.dtype != np.bool_ or L.shape[0] < 1:
        raise ValueError("labels must be a bool [permutations >= 1, m + n] array")
    P, N = L.shape
    W = (P + 63) // 64
    bits = np.zeros((N, W * 64), dtype=np.uint8)
    bits[:, :P] = L.T
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").reshape(N, W)


def unpack_perm_labels(packed, n_perms: int) -> np.ndarray:
    """The inverse of `pack_perm_labels`: uint64 [m + n, W] -> bool [n_perms, m + n] (bits past n_perms are dropped)."""
    packed = np.ascontiguousarray(packed, dtype="<u8")
    bits = np.unpackbits(packed.view(np.uint8).reshape(packed.shape[0], -1), axis=1, bitorder="little")
    return np.ascontiguousarray(bits[:, :int(n_perms)].T).astype(np.bool_)


def check_perm_labels(labels, m: int, n: int, n_perms: int) -> None:
    """ValueError unless `labels` describes `n_perms` relabellings of m + n pooled points with exactly m ones each: a bool
    [n_perms, m + n] array, or its packed form uint64 [m + n, (n_perms + 63) // 64] (`pack_perm_labels`; bits past n_perms are
    ignored).  The kernel's entry cannot make this check: it does not read device data on the host."""
    m, n, n_perms = int(m), int(n), int(n_perms)
    if m < 1 or n < 1:
        raise ValueError("both sample sets need at least one point")
    if n_perms < 1:
        raise ValueError("at least one permutation is needed, got %d" % n_perms)
    if not isinstance(labels, np.ndarray) or labels.ndim != 2 or labels.dtype not in (np.dtype(np.bool_), np.dtype(np.uint64)):
        raise ValueError("labels must be a bool [permutations, m + n] or a packed uint64 [m + n, words] numpy array")
    if labels.dtype == np.bool_:
        if labels.shape != (n_perms, m + n):
            raise ValueError("labels must be [%d, %d] (permutations, m + n), got %s" % (n_perms, m + n, tuple(labels.shape)))
        ones = labels.sum(axis=1)
    else:
        if labels.shape != (m + n, (n_perms + 63) // 64):
            raise ValueError("packed labels must be [%d, %d] (m + n, words), got %s"
                             % (m + n, (n_perms + 63) // 64, tuple(labels.shape)))
        ones = unpack_perm_labels(labels, n_perms).sum(axis=1)
    if np.any(ones != m):
        p = int(np.argmax(ones != m))
        raise ValueError("permutation %d labels %d points as the first set, not m = %d" % (p, int(ones[p]), m))


def _perm_count(labels, n_perms):
    """The number of permutations `labels` holds: its rows (bool) or `n_perms`, which the packed form needs."""
    if isinstance(labels, np.ndarray) and labels.ndim == 2 and labels.dtype == np.bool_:
        if n_perms is not None and int(n_perms) != labels.shape[0]:
            raise ValueError("n_perms = %d, but labels has %d rows" % (int(n_perms), labels.shape[0]))
        return int(labels.shape[0])
    if n_perms is None:
        raise ValueError("labels must be a bool [permutations, m + n] numpy array, or packed uint64 with n_perms given")
    return int(n_perms)


def mmd_perm_sums(X, Y, blocks: np.ndarray, xcols, ycols, labels, scale=None, wrap=None, device=None, n_perms=None):
    """The kernel sums {Sxx', Syy', Sxy'} of every block of `blocks` under every relabelling of the pooled set [X; Y]
    (X [m, x_cols], Y [n, y_cols], tensor or numpy): the null distribution of the MMD permutation test, every Gram value
    evaluated once for 256 permutations (nfisam_sample_mmd_perm).  `labels`: bool [P, m + n] numpy, row p marks the pooled
    points that count as the first set under permutation p (exactly m of them), or its packed form (`pack_perm_labels`) with
    `n_perms`; everything else as `mmd_sums`.  Every check comes before the first copy.
    -> [n_blocks, P, 3] float64 device tensor; [b, p] feeds `Statistics.mmd_from_sums` like a row of `mmd_sums`."""
    device = _row_major_front("mmd_perm_sums", device, X=X, Y=Y)
    check_mmd_blocks(blocks, xcols, ycols, int(X.shape[1]), int(Y.shape[1]), scale, wrap)
    check_perm_labels(labels, int(X.shape[0]), int(Y.shape[0]), _perm_count(labels, n_perms))
    return mmd_perm_sums_t(_columns(X, device), _columns(Y, device), blocks, xcols, ycols, labels, scale, wrap, checked=True,
                           n_perms=n_perms)


def mmd_perm_sums_t(Xt, Yt, blocks: np.ndarray, xcols, ycols, labels, scale=None, wrap=None, checked=False, n_perms=None):
    """`mmd_perm_sums` on the COLUMN-major matrices Xt [x_rows, m], Yt [y_rows, n] (contiguous float32 device tensors, used in
    place).  More than MMD_PERM_MAX permutations, or more than fit MMD_PERM_SCRATCH_BYTES of strip partials, are launched in
    chunks (multiples of 256) and concatenated: a permutation's numbers do not depend on the split."""
    Yt, x_rows, m, y_rows, n = _two_set_front(("Xt", "Yt"), Xt, Yt)
    device = Xt.device
    P = _perm_count(labels, n_perms)
    if not checked:
        check_mmd_blocks(blocks, xcols, ycols, x_rows, y_rows, scale, wrap)
        check_perm_labels(labels, m, n, P)
    nb = int(blocks.shape[0])
    blocks = np.ascontiguousarray(blocks)
    packed = pack_perm_labels(labels) if labels.dtype == np.bool_ else np.ascontiguousarray(labels)
    per_perm = int(lib().nfisam_sample_mmd_perm_scratch_count(m, n, nb, MMD_PERM_CHUNK)) // MMD_PERM_CHUNK * 8
    if per_perm < 1:
        raise ValueError("mmd_perm_sums: %d + %d points in %d blocks exceed the grid" % (m, n, nb))
    step = max(MMD_PERM_SCRATCH_BYTES // per_perm // MMD_PERM_CHUNK, 1) * MMD_PERM_CHUNK
    step = min(step, MMD_PERM_MAX)
    sums = torch.empty(nb, P, 3, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        dev, ne = _two_set_upload(device, blocks, ("xcols", "ycols"), xcols, ycols, scale=_entry_f64(scale), wrap=_flags(wrap))
        for p0 in range(0, P, step):
            cnt = min(step, P - p0)
            words = np.ascontiguousarray(packed[:, p0 // 64:(p0 + cnt + 63) // 64]).view(np.int64)
            lab = torch.from_numpy(words).to(device)
            count = int(lib().nfisam_sample_mmd_perm_scratch_count(m, n, nb, cnt))
            if count < 1:
                raise ValueError("mmd_perm_sums: %d + %d points, %d blocks and %d permutations exceed the grid" % (m, n, nb, cnt))
            scratch = torch.empty(count, dtype=torch.float64, device=device)
            out = sums if cnt == P else torch.empty(nb, cnt, 3, dtype=torch.float64, device=device)
            _check(lib().nfisam_sample_mmd_perm(_ptr(Xt), x_rows, m, _ptr(Yt), y_rows, n, blocks.ctypes.data_as(C.c_void_p),
                                                _ptr(dev["blocks"]), nb, _ptr(dev["xcols"]), _ptr(dev["ycols"]), ne,
                                                _ptr(dev["scale"]), _ptr(dev["wrap"]), _ptr(lab), cnt, _ptr(out), _ptr(scratch),
                                                _stream()), "nfisam_sample_mmd_perm")
            if out is not sums:
                sums[:, p0:p0 + cnt] = out
    return sums


# ---- the score of the joint density (nfisam_factor_graph_score) ------------------------------------------------------------------
def _slot_rows(terms: np.ndarray):
    """-> (slot_off [n_terms] int32, rows [n_slots] int64: the row of G every slot adds into), in table order: a factor writes
    one slot per row it touches, a's rows first, then b's or the candidates' (slot_count of csrc/factor_model.h)."""
    slot_off, rows = np.zeros(terms.shape[0], dtype=np.int32), []
    for i in range(terms.shape[0]):
        code, a, b, k = int(terms["code"][i]), int(terms["a"][i]), int(terms["b"][i]), int(terms["k"][i])
        slot_off[i] = len(rows)
        na, nb = _FAC_ROWS[code]
        rows += range(a, a + na)
        if code == FAC_CODES["RANGE_MIX"]:
            for c in terms["cand"][i, :k]:
                rows += (int(c), int(c) + 1)
        else:
            rows += range(b, b + nb)
    return slot_off, np.asarray(rows, dtype=np.int64)


def pack_score_gather(terms: np.ndarray, total_dim: int) -> dict:
    """The gather lists of `factor_graph_score` for the table `terms` (checked here: `check_factor_terms`):
    slot_off [n_terms] int32 (the first scratch slot of every factor), n_slots, and the CSR row_off [total_dim + 1] /
    row_slot [n_slots] int32: row r of G is the sum of the slots row_slot[row_off[r] : row_off[r + 1]], listed in table
    order (ascending slot index).  Every slot appears exactly once; a repeated candidate's slots land in the same rows."""
    check_factor_terms(terms, int(total_dim))
    slot_off, rows = _slot_rows(terms)
    order = np.argsort(rows, kind="stable")                            # by row; table order within a row
    row_off = np.zeros(int(total_dim) + 1, dtype=np.int32)
    row_off[1:] = np.cumsum(np.bincount(rows, minlength=int(total_dim)))
    return dict(slot_off=slot_off, n_slots=int(rows.size), row_off=row_off, row_slot=order.astype(np.int32))


def factor_graph_score(terms: np.ndarray, S, device, terms_dev=None, gather=None, slots=False):
    """G = d/dx log p(X, Z) at the n rows of S (nfisam_factor_graph_score): `terms` the numpy FACTOR_DTYPE table
    (`pack_factor_terms`), S [n, total_dim] in the walk's column layout (tensor or numpy; float32 points, the arithmetic
    is float64).  Launched on the current stream.  `terms_dev`: an uploaded copy of `terms` to reuse; `gather`: the result of
    `pack_score_gather(terms, total_dim)` to reuse.
    -> G [n, total_dim] float64 device tensor (a view of the column-major result); with slots=True: (G, slot values
    [n_slots, n] float64, the per-factor partial derivatives the rows are added from)."""
    total_dim = _points_width(S)
    if gather is None:
        gather = pack_score_gather(terms, total_dim)                   # (checks the table)
    out = factor_graph_score_t(terms, _columns(S, device), device, terms_dev=terms_dev, gather=gather, slots=slots)
    return (out[0].t(), out[1]) if slots else out.t()


def factor_graph_score_t(terms: np.ndarray, St, device, terms_dev=None, gather=None, slots=False):
    """`factor_graph_score` on the COLUMN-major matrix St [total_dim, n] (contiguous float32 device tensor): what the tree
    walk wrote, differentiated in place.  -> Gt [total_dim, n] float64 device tensor, the layout `ksd_sums_t` reads."""
    total_dim, n = _points_shape_t(St)
    if gather is None:
        gather = pack_score_gather(terms, total_dim)                   # (checks the table)
    elif gather["row_off"].shape[0] != total_dim + 1 or gather["slot_off"].shape[0] != terms.shape[0]:
        raise ValueError("gather was packed for another table or another total_dim")
    if total_dim > 65535:
        raise ValueError("factor_graph_score: at most 65535 rows are supported, got %d" % total_dim)
    nt, ns = int(terms.shape[0]), int(gather["n_slots"])
    Gt = torch.zeros(total_dim, n, dtype=torch.float64, device=device)
    vals = torch.empty(ns, n, dtype=torch.float64, device=device)     # the scratch: from torch's allocator
    if nt > 0 and n > 0:
        with torch.cuda.device(device):
            dev = _factor_tables(device, terms, terms_dev, slot_off=gather["slot_off"], row_off=gather["row_off"],
                                 row_slot=gather["row_slot"])
            assert int(lib().nfisam_factor_graph_score_scratch_count(ns, n)) == vals.numel()
            _check(lib().nfisam_factor_graph_score(_ptr(dev["terms"]), nt, _ptr(St), total_dim, n, _ptr(dev["slot_off"]), ns,
                                                   _ptr(dev["row_off"]), _ptr(dev["row_slot"]), _ptr(Gt), _ptr(vals),
                                                   _stream()), "nfisam_factor_graph_score")
    return (Gt, vals) if slots else Gt


# ---- Hessian-vector products of the joint density (nfisam_factor_graph_hvp) ------------------------------------------------------
def factor_graph_hvp(terms: np.ndarray, S, V, device, terms_dev=None, gather=None, score=False, slots=False):
    """H v at the n rows of S along the rows of V (nfisam_factor_graph_hvp): row p of the result is
    (d^2 log p / dx dx')(S_p) V_p.  `terms`, S, `terms_dev`, `gather`: as `factor_graph_score` takes them; V [n, total_dim]
    (tensor or numpy, brought to float64).  Launched on the current stream.
    -> H v [n, total_dim] float64 device tensor (a view of the column-major result); with score=True: (H v, G), G being
    `factor_graph_score`'s result bit for bit, from the same first pass; with slots=True the slot values [n_slots, n] of H v
    are appended."""
    total_dim = _points_width(S)
    if not (torch.is_tensor(V) or isinstance(V, np.ndarray)) or tuple(V.shape) != tuple(S.shape):
        raise ValueError("V must be a [n, total_dim] tensor or array of S's shape")
    if gather is None:
        gather = pack_score_gather(terms, total_dim)                   # (checks the table)
    Vt = V.to(device=device, dtype=torch.float64).t().contiguous() if torch.is_tensor(V) else \
        torch.from_numpy(np.ascontiguousarray(V.T, dtype=np.float64)).to(device)
    out = factor_graph_hvp_t(terms, _columns(S, device), Vt, device, terms_dev=terms_dev, gather=gather, score=score, slots=slots)
    if not (score or slots):
        return out.t()
    return tuple(o.t() if i < 1 + bool(score) else o for i, o in enumerate(out))


def factor_graph_hvp_t(terms: np.ndarray, St, Vt, device, terms_dev=None, gather=None, score=False, slots=False):
    """`factor_graph_hvp` on the COLUMN-major matrices St [total_dim, n] (contiguous float32 device tensor) and Vt (contiguous
    float64 tensor of St's shape on St's device: ValueError otherwise, before any launch).
    -> Ht [total_dim, n] float64; with score=True: (Ht, Gt); with slots=True the slot values of H v are appended."""
    total_dim, n = _points_shape_t(St)
    if not torch.is_tensor(Vt) or Vt.dtype != torch.float64 or not Vt.is_contiguous() or tuple(Vt.shape) != (total_dim, n):
        raise ValueError("Vt must be a contiguous float64 [total_dim, n] tensor of St's shape")
    if Vt.device != St.device:
        raise ValueError("St and Vt must be on the same device")
    if gather is None:
        gather = pack_score_gather(terms, total_dim)                   # (checks the table)
    elif gather["row_off"].shape[0] != total_dim + 1 or gather["slot_off"].shape[0] != terms.shape[0]:
        raise ValueError("gather was packed for another table or another total_dim")
    if total_dim > 65535:
        raise ValueError("factor_graph_hvp: at most 65535 rows are supported, got %d" % total_dim)
    nt, ns = int(terms.shape[0]), int(gather["n_slots"])
    Ht = torch.zeros(total_dim, n, dtype=torch.float64, device=device)
    Gt = torch.zeros(total_dim, n, dtype=torch.float64, device=device) if score else None
    vals = torch.empty((2 if score else 1) * ns, n, dtype=torch.float64, device=device)      # the scratch: H v's slots, then G's
    if nt > 0 and n > 0:
        with torch.cuda.device(device):
            dev = _factor_tables(device, terms, terms_dev, slot_off=gather["slot_off"], row_off=gather["row_off"],
                                 row_slot=gather["row_slot"])
            assert int(lib().nfisam_factor_graph_hvp_scratch_count(ns, n, int(bool(score)))) == vals.numel()
            _check(lib().nfisam_factor_graph_hvp(_ptr(dev["terms"]), nt, _ptr(St), _ptr(Vt), total_dim, n, _ptr(dev["slot_off"]),
                                                 ns, _ptr(dev["row_off"]), _ptr(dev["row_slot"]), _ptr(Ht),
                                                 _ptr(Gt) if score else None, _ptr(vals), _stream()), "nfisam_factor_graph_hvp")
    out = (Ht,) + ((Gt,) if score else ()) + ((vals[:ns],) if slots else ())
    return out if len(out) > 1 else Ht


# ---- kernel Stein discrepancy: the pairwise Stein sums (nfisam_sample_ksd) ----------------------------------------------------------
KSD_MATRIX_MAX_N = 4096                                               # NFISAM_KSD_MATRIX_MAX_N


def check_ksd_args(rows: int, n: int, g_shape, precision, wrap=None, matrix=False) -> None:
    """ValueError for what the kernel must not see: no point, a score matrix of another shape than the points', a precision
    that is not one finite value >= 0 per column, flags of another length, the matrix for more than 4096 points."""
    if n < 1 or rows < 1:
        raise ValueError("ksd_sums needs at least one point and one column")
    if tuple(g_shape) != (rows, n):
        raise ValueError("the score matrix must have the shape of the points: %s, got %s" % ((rows, n), tuple(g_shape)))
    p = precision.detach().cpu().numpy() if torch.is_tensor(precision) else np.asarray(precision, dtype=np.float64)
    if p.shape != (rows,):
        raise ValueError("precision must have one value per column (%d)" % rows)
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        raise ValueError("precision must be finite and >= 0")
    if wrap is not None and np.shape(wrap) != (rows,):
        raise ValueError("wrap must have one flag per column (%d)" % rows)
    if matrix and n > KSD_MATRIX_MAX_N:
        raise ValueError("the matrix H is returned for at most %d points, got %d" % (KSD_MATRIX_MAX_N, n))


def ksd_sums(X, G, precision, wrap=None, matrix=False, device=None):
    """The Stein sums of the points X [n, D] (tensor or numpy; float32 points) with scores G [n, D] (float64) under the
    Gaussian kernel of DIAGONAL precision `precision` [D] >= 0 (nfisam_sample_ksd, on the current stream); wrap [D] marks
    angles (differences brought into [-pi, pi]).
    -> {"row": [n] sum_j h_ij over all j, "diag": [n] h_ii, "H": [n, n] with matrix=True (n <= 4096), else None}, float64
    device tensors.  `Statistics.ksd_from_sums` forms the U- and V-statistics."""
    device = _row_major_front("ksd_sums", device, X=X, G=G)
    check_ksd_args(int(X.shape[1]), int(X.shape[0]), (int(G.shape[1]), int(G.shape[0])), precision, wrap, matrix)
    Gt = G.to(device=device, dtype=torch.float64).t().contiguous() if torch.is_tensor(G) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(G, dtype=np.float64).T)).to(device)
    return ksd_sums_t(_columns(X, device), Gt, precision, wrap, matrix, checked=True)


def ksd_sums_t(Xt, Gt, precision, wrap=None, matrix=False, checked=False):
    """`ksd_sums` on the COLUMN-major matrices Xt [D, n] (contiguous float32) and Gt [D, n] (contiguous float64) on one
    ROCm device, used in place: the tree walk's St and `factor_graph_score_t`'s result."""
    rows, n = _column_major_front("Xt", Xt)
    _score_front("Gt", Gt, Xt)
    if not checked:
        check_ksd_args(rows, n, tuple(Gt.shape), precision, wrap, matrix)
    device = Xt.device
    with torch.cuda.device(device):
        dev = _upload_named(device, precision=_entry_f64(precision), wrap=_flags(wrap))
        count = int(lib().nfisam_sample_ksd_scratch_count(n))
        if count < 1:
            raise ValueError("ksd_sums: %d points exceed the grid" % n)
        scratch = torch.empty(count, dtype=torch.float64, device=device)
        row = torch.empty(n, dtype=torch.float64, device=device)
        diag = torch.empty(n, dtype=torch.float64, device=device)
        H = torch.empty(n, n, dtype=torch.float64, device=device) if matrix else None
        _check(lib().nfisam_sample_ksd(_ptr(Xt), _ptr(Gt), rows, n, _ptr(dev["precision"]), _ptr(dev["wrap"]), _ptr(row),
                                       _ptr(diag), _ptr(H), _ptr(scratch), _stream()), "nfisam_sample_ksd")
    return dict(row=row, diag=diag, H=H)


# ---- Stein variational direction and step: the samples moved along the score (nfisam_sample_svgd, nfisam_sample_step) ----------
def check_svgd_blocks(blocks: np.ndarray, cols, x_rows: int, scale=None, wrap=None) -> None:
    """ValueError for tables the kernels must not see: what `check_mmd_blocks` refuses (no block or more than 65535, d < 1, a
    bandwidth term that is not positive and finite, entries outside [0, n_entries), a row outside [0, x_rows), per-entry arrays
    of another length, a scale that is not finite), two blocks that share an entry, and a row of Xt named more than once: a
    column has one direction.  (A device tensor's length alone is checked: checking its values would read it back.)"""
    named = {"cols": (cols, x_rows)}
    off, d = _check_table_layout(blocks, MMD_BLOCK_DTYPE, "MMD_BLOCK_DTYPE", named, dict(scale=scale, wrap=wrap))
    _check_disjoint(off, d, "the direction is stored by entry")
    _check_bandwidths(blocks)
    _check_rows(named)
    c = np.asarray(cols)
    if np.unique(c).size != c.size:
        raise ValueError("cols: a row of Xt is named more than once: a column has one direction")
    if scale is not None and not (torch.is_tensor(scale) and scale.is_cuda) and \
            not np.all(np.isfinite(np.asarray(scale, dtype=np.float64))):
        raise ValueError("scale must be finite")


def svgd_tables(device, blocks: np.ndarray, cols, scale=None, wrap=None, eps=None) -> dict:
    """The tables of `svgd_direction_t` / `sample_step_t` on `device`, one upload, to reuse over the steps of a loop:
    {"host": the contiguous block table, "blocks", "cols", "scale", "wrap", "eps": device tensors or None, "n_entries"}."""
    blocks = np.ascontiguousarray(blocks)
    c = np.asarray(cols, dtype=np.int32)
    dev = _upload_named(device, blocks=_table_bytes(blocks), cols=c, scale=_entry_f64(scale), wrap=_flags(wrap),
                        eps=_entry_f64(eps))
    return dict(dev, host=blocks, n_entries=int(c.size))


def svgd_direction(X, G, blocks: np.ndarray, cols, scale=None, wrap=None, device=None):
    """The Stein variational direction of the points X [n, x_cols] (tensor or numpy; float32 points) with scores G [n, x_cols]
    (float64) for every block of `blocks` (nfisam_sample_svgd, on the current stream): `blocks` numpy MMD_BLOCK_DTYPE
    (`pack_mmd_blocks`: widths and bandwidths; no two blocks share an entry), entry e is column cols[e] of X and of G (no
    column twice); scale [n_entries] multiplies an entry's differences in the kernel (0: the column leaves it and still gets
    its kernel-weighted mean score), wrap [n_entries] marks angles (differences brought into [-pi, pi]).
    -> Phi [n_entries, n] float64 device tensor:
    Phi[e, i] = sum_j k_b(i, j) (G[j, cols[e]] + 2 inv_two_sigma2 scale_e^2 (x_i - x_j)_e) / n."""
    device = _row_major_front("svgd_direction", device, X=X, G=G)
    if tuple(G.shape) != tuple(X.shape):
        raise ValueError("the score matrix must have the shape of the points: %s, got %s" % (tuple(X.shape), tuple(G.shape)))
    if int(X.shape[0]) < 1:
        raise ValueError("svgd_direction: no points")
    check_svgd_blocks(blocks, cols, int(X.shape[1]), scale, wrap)
    Gt = G.to(device=device, dtype=torch.float64).t().contiguous() if torch.is_tensor(G) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(G, dtype=np.float64).T)).to(device)
    return svgd_direction_t(_columns(X, device), Gt, blocks, cols, scale, wrap, checked=True)


def svgd_direction_t(Xt, Gt, blocks: np.ndarray, cols, scale=None, wrap=None, checked=False, tables=None):
    """`svgd_direction` on the COLUMN-major matrices Xt [x_rows, n] (contiguous float32) and Gt [x_rows, n] (contiguous
    float64) on one ROCm device, used in place: the tree walk's St and `factor_graph_score_t`'s result.  `tables`: the result
    of `svgd_tables` for the same arguments, to reuse over the steps of a loop."""
    x_rows, n = _column_major_front("Xt", Xt)
    _score_front("Gt", Gt, Xt)
    if tuple(Gt.shape) != (x_rows, n):
        raise ValueError("the score matrix must have the shape of the points: %s, got %s" % ((x_rows, n), tuple(Gt.shape)))
    if n < 1:
        raise ValueError("svgd_direction: no points")
    if not checked:
        check_svgd_blocks(blocks, cols, x_rows, scale, wrap)
    device = Xt.device
    with torch.cuda.device(device):
        t = tables if tables is not None else svgd_tables(device, blocks, cols, scale, wrap)
        nb, ne = int(t["host"].shape[0]), t["n_entries"]
        count = int(lib().nfisam_sample_svgd_scratch_count(n, nb, ne))
        if count < 1:
            raise ValueError("svgd_direction: %d points in %d blocks exceed the grid" % (n, nb))
        scratch = torch.empty(count, dtype=torch.float64, device=device)       # the per-tile partials: torch's allocator
        Phi = torch.zeros(ne, n, dtype=torch.float64, device=device)           # (an entry no block owns keeps its zero)
        _check(lib().nfisam_sample_svgd(_ptr(Xt), x_rows, n, _ptr(Gt), t["host"].ctypes.data_as(C.c_void_p), _ptr(t["blocks"]),
                                        nb, _ptr(t["cols"]), ne, _ptr(t["scale"]), _ptr(t["wrap"]), _ptr(Phi), _ptr(scratch),
                                        _stream()), "nfisam_sample_svgd")
    return Phi


def check_step_args(alpha, fudge, eps=None) -> None:
    """ValueError for what nfisam_sample_step refuses (alpha outside [0, 1), a fudge that is not positive and finite) and for
    host step lengths that are not finite."""
    if not (np.isfinite(alpha) and 0.0 <= alpha < 1.0):
        raise ValueError("alpha must lie in [0, 1), got %r" % (alpha,))
    if not (np.isfinite(fudge) and fudge > 0):
        raise ValueError("fudge must be positive and finite, got %r" % (fudge,))
    if eps is not None and not (torch.is_tensor(eps) and eps.is_cuda) and not np.all(np.isfinite(np.asarray(eps, dtype=np.float64))):
        raise ValueError("eps must be finite")


def sample_step_t(Xt, cols, Phi, hist, eps, wrap=None, alpha=0.9, fudge=1e-6, first=False, checked=False, tables=None):
    """One step of the points Xt [x_rows, n] (contiguous float32 device matrix) along the direction Phi [n_entries, n]
    (float64, as `svgd_direction_t` returns it), IN PLACE (nfisam_sample_step, on the current stream):
        hist = phi^2 if first else alpha hist + (1 - alpha) phi^2;  x += eps[e] phi / (sqrt(hist) + fudge)
    in float64, rounded to float32, entry e being row cols[e] of Xt (no row twice); wrap [n_entries] marks angles, which are
    brought back into [-pi, pi).  hist [n_entries, n] float64: the caller's state, updated in place; eps [n_entries]: one step
    length per entry in the column's own unit.  A step below the float32 spacing of a coordinate is lost (7.6e-6 at 100 m).
    `tables`: the result of `svgd_tables(..., eps=eps)` to reuse.  -> None."""
    x_rows, n = _column_major_front("Xt", Xt)
    ne = int(tables["n_entries"]) if tables is not None else int(np.size(cols))
    for name, t in (("Phi", Phi), ("hist", hist)):
        _score_front(name, t, Xt)
        if tuple(t.shape) != (ne, n):
            raise ValueError("%s must be [n_entries, n] = %s, got %s" % (name, (ne, n), tuple(t.shape)))
    if n < 1 or ne < 1:
        raise ValueError("sample_step: no points or no entries")
    if not checked:
        c = np.asarray(cols)
        if c.ndim != 1:
            raise ValueError("cols must be a 1-D list of at least one row")
        _check_rows({"cols": (c, x_rows)})
        if np.unique(c).size != c.size:
            raise ValueError("cols: a row of Xt is named more than once: a column has one direction")
        for name, a in (("eps", eps), ("wrap", wrap)):
            if a is not None and (tuple(a.shape) if torch.is_tensor(a) else np.shape(a)) != (ne,):
                raise ValueError("%s must have one %s per entry (%d)" % (name, "flag" if name == "wrap" else "value", ne))
        if eps is None:
            raise ValueError("eps must have one value per entry (%d)" % ne)
        check_step_args(alpha, fudge, eps)
    device = Xt.device
    with torch.cuda.device(device):
        t = tables if tables is not None else _upload_named(device, cols=np.asarray(cols, dtype=np.int32), wrap=_flags(wrap),
                                                            eps=_entry_f64(eps))
        _check(lib().nfisam_sample_step(_ptr(Xt), x_rows, n, _ptr(t["cols"]), ne, _ptr(t["wrap"]), _ptr(Phi), _ptr(hist),
                                        _ptr(t["eps"]), C.c_double(float(alpha)), C.c_double(float(fudge)), C.c_int(int(bool(first))),
                                        _stream()), "nfisam_sample_step")


# ---- Metropolis-corrected moves: the Langevin / random-walk proposal and the accept step (nfisam_sample_propose / _accept) -----
MCMC_SLAB = 32                                                        # rows per slab of the accept step's row sum (sample_mcmc.hip)
MCMC_MAX_N, MCMC_MAX_ROWS = 65535 * 64, 65535 * MCMC_SLAB


def check_mcmc_args(x_rows: int, n: int, h, wrap=None, seed=0, t=0) -> None:
    """ValueError for what nfisam_sample_propose / nfisam_sample_accept refuse (no rows, no chains, more than 65535 * 64 chains or
    65535 * 32 rows) and for what they do not read on the host: `h` must hold one finite step length >= 0 per row (a device tensor's
    length alone is checked: checking its values would read it back), `wrap` one flag per row; `seed` an integer in [0, 2^64), `t`
    one in [0, 2^32): the words of the generator's key and counter."""
    if not (1 <= int(x_rows) <= MCMC_MAX_ROWS and 1 <= int(n) <= MCMC_MAX_N):
        raise ValueError("1..%d rows and 1..%d chains are supported, got %d and %d" % (MCMC_MAX_ROWS, MCMC_MAX_N, x_rows, n))
    if h is None:
        raise ValueError("h must have one value per row (%d)" % x_rows)
    for name, a in (("h", h), ("wrap", wrap)):
        if a is not None and (tuple(a.shape) if torch.is_tensor(a) else np.shape(a)) != (int(x_rows),):
            raise ValueError("%s must have one %s per row (%d)" % (name, "flag" if name == "wrap" else "value", x_rows))
    if not (torch.is_tensor(h) and h.is_cuda):
        hv = np.asarray(h, dtype=np.float64)
        if not np.all(np.isfinite(hv) & (hv >= 0)):
            raise ValueError("h must be finite and >= 0 (0 freezes a row)")
    for name, v, top in (("seed", seed, 1 << 64), ("t", t, 1 << 32)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < top:
            raise ValueError("%s must be an integer in [0, 2^%d), got %r" % (name, 64 if name == "seed" else 32, v))


def mcmc_tables(device, h, wrap=None) -> dict:
    """The per-row arrays of `sample_propose_t` / `sample_accept_t` on `device`, one upload, to reuse over the steps of a chain:
    {"h": float64 [x_rows], "wrap": uint8 [x_rows] or None}."""
    return _upload_named(device, h=_entry_f64(h), wrap=_flags(wrap))


def _mcmc_front(Xt, mats, h, wrap, seed, t, checked, tables):
    """What the two bindings share: the points, every other matrix of `mats` ({name: (tensor or None, dtype)}) of their shape on
    their device, the argument checks -> (x_rows, n)."""
    x_rows, n = _column_major_front("Xt", Xt)
    for name, (M, dtype) in mats.items():
        if M is None:
            continue
        if dtype == torch.float32:
            _column_major_front(name, M)
            if M.device != Xt.device:
                raise ValueError("Xt and %s must be on the same device" % name)
        else:
            _score_front(name, M, Xt)
        if tuple(M.shape) != (x_rows, n):
            raise ValueError("%s must have the shape of the points: %s, got %s" % (name, (x_rows, n), tuple(M.shape)))
    if not checked:
        check_mcmc_args(x_rows, n, tables["h"] if tables is not None else h, tables["wrap"] if tables is not None else wrap,
                        seed, t)
    return x_rows, n


def sample_propose_t(Xt, Gx, h, wrap=None, seed=0, t=0, Yt=None, checked=False, tables=None):
    """The Metropolis proposal of the n chains in the COLUMN-major device matrix Xt [x_rows, n] (contiguous float32)
    (nfisam_sample_propose, on the current stream): y = x + (h_r^2 / 2) g + h_r z in float64 with Gx [x_rows, n] (float64, as
    `factor_graph_score_t` returns it; None: the random walk y = x + h_r z), h [x_rows] the step length of a row in its own
    unit (0: the row is copied bit for bit), wrap [x_rows] marks angles (brought into [-pi, pi)).  z are the normals of the
    generator contract: Philox4x32-10 keyed by `seed`, counter (chain, row >> 2, `t`, 0) -- the same for a chain at any n.
    `Yt`: the matrix to write (default: a new one); `tables`: the result of `mcmc_tables` to reuse.  Xt is not written.
    -> Yt [x_rows, n] float32."""
    x_rows, n = _mcmc_front(Xt, {"Gx": (Gx, torch.float64), "Yt": (Yt, torch.float32)}, h, wrap, seed, t, checked, tables)
    device = Xt.device
    with torch.cuda.device(device):
        tb = tables if tables is not None else mcmc_tables(device, h, wrap)
        if Yt is None:
            Yt = torch.empty_like(Xt)
        _check(lib().nfisam_sample_propose(_ptr(Xt), _ptr(Gx), _ptr(Yt), x_rows, n, _ptr(tb["h"]), _ptr(tb["wrap"]),
                                           C.c_uint64(int(seed)), C.c_uint32(int(t)), _stream()), "nfisam_sample_propose")
    return Yt


def sample_accept_scratch(x_rows: int, n: int, device):
    """The scratch of `sample_accept_t` for this shape (nfisam_sample_accept_scratch_count doubles), to reuse over the steps."""
    count = int(lib().nfisam_sample_accept_scratch_count(int(x_rows), int(n)))
    if count < 1:
        raise ValueError("sample_accept: %d rows and %d chains exceed the grid" % (x_rows, n))
    return torch.empty(count, dtype=torch.float64, device=device)


def sample_accept_t(Xt, Yt, Gx, Gy, lp_x, lp_y, h, wrap=None, seed=0, t=0, checked=False, tables=None, scratch=None):
    """The accept / reject step of the n chains Xt [x_rows, n] against their proposals Yt (nfisam_sample_accept, on the current
    stream), IN PLACE: log alpha = (lp_y - lp_x) + the log ratio of the Langevin proposal densities there and back, from the
    float32 values stored in Xt and Yt and the scores Gx, Gy [x_rows, n] float64 at them (both None: a symmetric proposal, no
    ratio -- the random walk, or an independence step with lp = log p - log q); lp_x, lp_y [n] float64.  A chain accepts iff
    log(u) < log alpha, u the uniform of counter (chain, 0, `t`, 1) under `seed`; then its column of Yt, Gy and its lp_y replace
    those of Xt, Gx and lp_x.  A rejected chain keeps every bit; a NaN log alpha or lp_y = -inf rejects.
    -> (log_alpha [n] float64, accepted [n] uint8) on the device."""
    x_rows, n = _mcmc_front(Xt, {"Yt": (Yt, torch.float32), "Gx": (Gx, torch.float64), "Gy": (Gy, torch.float64)}, h, wrap, seed,
                            t, checked, tables)
    if (Gx is None) != (Gy is None):
        raise ValueError("Gx and Gy go together: both scores, or neither (a symmetric proposal)")
    for name, v in (("lp_x", lp_x), ("lp_y", lp_y)):
        if not torch.is_tensor(v) or not v.is_cuda:
            raise RuntimeError("%s must be a tensor on a ROCm device (no CPU path exists)" % name)
        if v.dtype != torch.float64 or tuple(v.shape) != (n,) or not v.is_contiguous() or v.device != Xt.device:
            raise ValueError("%s must be a contiguous float64 [n] = (%d,) tensor on Xt's device" % (name, n))
    device = Xt.device
    with torch.cuda.device(device):
        tb = tables if tables is not None else mcmc_tables(device, h, wrap)
        if scratch is None:
            scratch = sample_accept_scratch(x_rows, n, device)
        log_alpha = torch.empty(n, dtype=torch.float64, device=device)
        accepted = torch.empty(n, dtype=torch.uint8, device=device)
        _check(lib().nfisam_sample_accept(_ptr(Xt), _ptr(Yt), _ptr(Gx), _ptr(Gy), _ptr(lp_x), _ptr(lp_y), x_rows, n, _ptr(tb["h"]),
                                          _ptr(tb["wrap"]), C.c_uint64(int(seed)), C.c_uint32(int(t)), _ptr(log_alpha),
                                          _ptr(accepted), _ptr(scratch), _stream()), "nfisam_sample_accept")
    return log_alpha, accepted


def sample_propose(X, G, h, wrap=None, seed=0, t=0, device=None):
    """`sample_propose_t` for row-major points X [n, x_cols] (tensor or numpy) and scores G [n, x_cols] (or None)
    -> Y [n, x_cols] float32 device tensor."""
    mats = dict(X=X) if G is None else dict(X=X, G=G)
    device = _row_major_front("sample_propose", device, **mats)
    if G is not None and tuple(G.shape) != tuple(X.shape):
        raise ValueError("the score matrix must have the shape of the points: %s, got %s" % (tuple(X.shape), tuple(G.shape)))
    check_mcmc_args(int(X.shape[1]), int(X.shape[0]), h, wrap, seed, t)
    Gt = None if G is None else _f64(G, device).t().contiguous()
    return sample_propose_t(_columns(X, device), Gt, h, wrap, seed, t, checked=True).t().contiguous()


# ---- chain diagnostics: the streaming fold of the chains' states and the per-row finish (nfisam_chain_record / _finish) --------
CHAIN_MAX_LEVELS = 16                                                 # NFISAM_CHAIN_MAX_LEVELS


def chain_max_levels(T: int) -> int:
    """The most blocking levels a run of T recorded states takes: min(16, floor(log2 T)), every level with at least two blocks."""
    return min(CHAIN_MAX_LEVELS, int(T).bit_length() - 1)


def check_chain_args(x_rows: int, n: int, levels, T, t=0, center=None, wrap=None) -> None:
    """ValueError for what nfisam_chain_record / nfisam_chain_finish refuse (no rows, no chains, more than 65535 * 64 chains, an
    odd T or one below 2, t outside [0, T), levels outside [1, min(16, floor(log2 T))]) and for what they do not read on the
    host: `center` must hold one finite value per row (a device tensor's length alone is checked), `wrap` one flag per row."""
    if not (int(x_rows) >= 1 and 1 <= int(n) <= MCMC_MAX_N):
        raise ValueError("at least 1 row and 1..%d chains are supported, got %d and %d" % (MCMC_MAX_N, x_rows, n))
    for name, v in (("T", T), ("t", t), ("levels", levels)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not (2 <= int(T) < 1 << 32) or int(T) % 2:
        raise ValueError("T, the number of recorded states, must be even and in [2, 2^32), got %d" % T)
    if not 0 <= int(t) < int(T):
        raise ValueError("t must lie in [0, T = %d), got %d" % (T, t))
    if not 1 <= int(levels) <= chain_max_levels(T):
        raise ValueError("levels must lie in [1, min(16, floor(log2 T)) = %d] for T = %d, got %d" % (chain_max_levels(T), T, levels))
    for name, a in (("center", center), ("wrap", wrap)):
        if a is not None and (tuple(a.shape) if torch.is_tensor(a) else np.shape(a)) != (int(x_rows),):
            raise ValueError("%s must have one %s per row (%d)" % (name, "flag" if name == "wrap" else "value", x_rows))
    if center is not None and not (torch.is_tensor(center) and center.is_cuda):
        if not np.all(np.isfinite(np.asarray(center, dtype=np.float64))):
            raise ValueError("center must be finite")


def chain_tables(device, center=None, wrap=None) -> dict:
    """The per-row arrays of `chain_record_t` / `chain_finish_t` on `device`, one upload, to reuse over the steps of a run:
    {"center": float64 [x_rows] or None, "wrap": uint8 [x_rows] or None}."""
    return _upload_named(device, center=_entry_f64(center), wrap=_flags(wrap))


def chain_state(D: int, n: int, levels: int, device):
    """The zeroed accumulators of `chain_record_t` for D rows, n chains and `levels` blocking levels: float64
    [4 + 3 (levels - 1), D, n] on `device` (nfisam_chain_state_count doubles, slot-major)."""
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (D, n, levels)):
        raise ValueError("D, n and levels must be integers")
    if not (int(D) >= 1 and 1 <= int(n) <= MCMC_MAX_N and 1 <= int(levels) <= CHAIN_MAX_LEVELS):
        raise ValueError("chain_state: at least 1 row, 1..%d chains and 1..%d levels are supported, got %d, %d and %d"
                         % (MCMC_MAX_N, CHAIN_MAX_LEVELS, D, n, levels))
    if torch.device(device).type != "cuda":
        raise RuntimeError("chain_state needs a ROCm device (no CPU path exists)")
    slots = 4 + 3 * (int(levels) - 1)
    assert int(lib().nfisam_chain_state_count(int(D), int(n), int(levels))) == slots * int(D) * int(n)
    return torch.zeros(slots, int(D), int(n), dtype=torch.float64, device=device)


def _chain_state_front(state, x_rows, n, levels, device):
    if not torch.is_tensor(state) or not state.is_cuda:
        raise RuntimeError("state must be a tensor on a ROCm device (no CPU path exists)")
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)):
        raise ValueError("levels must be an integer, got %r" % (levels,))
    want = (4 + 3 * (int(levels) - 1), x_rows, n)
    if state.dtype != torch.float64 or tuple(state.shape) != want or not state.is_contiguous() or state.device != device:
        raise ValueError("state must be the contiguous float64 %s tensor of `chain_state` on the points' device" % (want,))


def chain_record_t(state, Xt, t, T, levels, center=None, wrap=None, tables=None, checked=False):
    """Fold the current state of the n chains in the COLUMN-major device matrix Xt [x_rows, n] (contiguous float32) into the
    accumulators `state` of `chain_state` (nfisam_chain_record, on the current stream): recorded state number t of T, one call
    per t = 0 ... T - 1, ascending.  The value recorded for row r is the float64 deviation x - center[r], wrapped into [-pi, pi)
    where wrap[r] is set; center None: 0.  `tables`: the result of `chain_tables` to reuse.  Xt is not written.  -> state."""
    x_rows, n = _column_major_front("Xt", Xt)
    if not checked:
        check_chain_args(x_rows, n, levels, T, t, tables["center"] if tables is not None else center,
                         tables["wrap"] if tables is not None else wrap)
    _chain_state_front(state, x_rows, n, levels, Xt.device)
    device = Xt.device
    with torch.cuda.device(device):
        tb = tables if tables is not None else chain_tables(device, center, wrap)
        _check(lib().nfisam_chain_record(_ptr(Xt), _ptr(state), x_rows, n, int(levels), _ptr(tb["center"]), _ptr(tb["wrap"]),
                                         C.c_uint32(int(t)), C.c_uint32(int(T)), _stream()), "nfisam_chain_record")
    return state


def chain_finish_t(state, D, n, levels, T, center=None, wrap=None, tables=None):
    """The per-row statistics of the T states recorded in `state` (nfisam_chain_finish, on the current stream), with the
    `center` and `wrap` of the record calls (or their `tables`)
    -> dict(mean [D], within [D], rhat [D], tau [levels, D]) of float64 device tensors: the mean over chains and states (the
    centre added back, wrapped on a circular row), the pooled within-chain variance, split-R-hat over the 2 n half-chains
    (NaN for T < 4 and on a row without spread) and the blocking estimates of the integrated autocorrelation time at block
    lengths 1, 2, ..., 2^(levels - 1) (`Statistics.blocking_tau` picks the one to quote)."""
    if not torch.is_tensor(state) or not state.is_cuda:
        raise RuntimeError("state must be a tensor on a ROCm device (no CPU path exists)")
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (D, n)):
        raise ValueError("D and n must be integers")
    device = state.device
    _chain_state_front(state, int(D), int(n), levels, device)
    check_chain_args(int(D), int(n), levels, T, 0, tables["center"] if tables is not None else center,
                     tables["wrap"] if tables is not None else wrap)
    with torch.cuda.device(device):
        tb = tables if tables is not None else chain_tables(device, center, wrap)
        out = torch.empty(3 + int(levels), int(D), dtype=torch.float64, device=device)
        _check(lib().nfisam_chain_finish(_ptr(state), int(D), int(n), int(levels), C.c_uint32(int(T)), _ptr(tb["center"]),
                                         _ptr(tb["wrap"]), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3:]), _stream()),
               "nfisam_chain_finish")
    return dict(mean=out[0], within=out[1], rhat=out[2], tau=out[3:])


# ---- sample summaries: means, resultant lengths, covariances, quantiles (nfisam_sample_moments, nfisam_sample_quantiles) --------
MOMENT_BLOCK_DTYPE = np.dtype([("col_off", np.int32), ("d", np.int32), ("cov_off", np.int64)])
assert MOMENT_BLOCK_DTYPE.itemsize == C.sizeof(MomentBlock)


def pack_moment_blocks(dims) -> np.ndarray:
    """The block table (numpy MOMENT_BLOCK_DTYPE) of consecutive blocks of `dims` entries, their d x d matrices one after
    another in `cov`."""
    dims, t = _consecutive(dims, MOMENT_BLOCK_DTYPE)
    t["cov_off"] = np.cumsum(dims * dims) - dims * dims
    return t


def check_moment_blocks(blocks: np.ndarray, cols, x_rows: int, circular=None, cov_count: int = None) -> None:
    """ValueError for tables the kernel must not see: no block or more than 65535, d outside 1..16, entries outside
    [0, n_entries), a matrix outside [0, cov_count) (default: the end of the last matrix), a row outside [0, x_rows), flags of
    another length."""
    cols = {"cols": (cols, x_rows)}
    off, d = _check_table_layout(blocks, MOMENT_BLOCK_DTYPE, "MOMENT_BLOCK_DTYPE", cols, dict(circular=circular), MOMENTS_MAX_D)
    coff = blocks["cov_off"].astype(np.int64)
    count = int((coff + d * d).max()) if cov_count is None else int(cov_count)
    bad = (coff < 0) | (coff + d * d > count)
    if np.any(bad):
        raise ValueError("block %d: its matrix at %d leaves the %d values of cov" % (int(np.argmax(bad)), int(coff[np.argmax(bad)]), count))
    _check_rows(cols)


def _check_weights(weights, n):
    """None, or float64 [n] weights (tensor or numpy): non-negative, finite, not all zero.  A device tensor is taken as it is
    (checking it would read it back): its length and dtype alone are checked."""
    if weights is None:
        return None
    if torch.is_tensor(weights) and weights.is_cuda:
        if weights.ndim != 1 or int(weights.shape[0]) != n:
            raise ValueError("weights must be [n] = [%d], got %s" % (n, tuple(weights.shape)))
        return weights
    w = weights.detach().numpy() if torch.is_tensor(weights) else np.asarray(weights)
    if w.ndim != 1 or w.size != n:
        raise ValueError("weights must be [n] = [%d], got %s" % (n, tuple(w.shape)))
    w = w.astype(np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0) or not np.any(w > 0):
        raise ValueError("weights must be finite, non-negative and not all zero")
    return w


def sample_moments(X, blocks: np.ndarray, cols, circular=None, weights=None, device=None):
    """Means, resultant lengths and covariances of every block of `blocks` over the n rows of X [n, x_cols] (tensor or numpy;
    float32 points, float64 arithmetic): nfisam_sample_moments, all blocks in one call on the current stream.  `blocks`: numpy
    MOMENT_BLOCK_DTYPE (`pack_moment_blocks`); entry e is column cols[e] of X; circular [n_entries] marks angles (circular mean
    in [-pi, pi), residuals wrapped); weights [n] float64 (None: all ones).
    -> (mean [n_entries], resultant [n_entries] (NaN for a Euclidean entry), cov [sum d^2], block b's row-major d x d matrix
    at blocks["cov_off"][b]): float64 device tensors."""
    device = _row_major_front("sample_moments", device, X=X)
    if int(X.shape[0]) < 1:
        raise ValueError("sample_moments: no points")
    check_moment_blocks(blocks, cols, int(X.shape[1]), circular)
    weights = _check_weights(weights, int(X.shape[0]))
    return sample_moments_t(_columns(X, device), blocks, cols, circular, weights, checked=True)


def sample_moments_t(Xt, blocks: np.ndarray, cols, circular=None, weights=None, checked=False):
    """`sample_moments` on the COLUMN-major matrix Xt [x_rows, n] (a contiguous float32 device tensor, used in place): what
    the tree walk wrote.  `checked` skips the table check (the caller has made it)."""
    x_rows, n = _column_major_front("Xt", Xt)
    device = Xt.device
    if n < 1:
        raise ValueError("sample_moments: no points")
    if not checked:
        check_moment_blocks(blocks, cols, x_rows, circular)
        weights = _check_weights(weights, n)
    nb = int(blocks.shape[0])
    cc = np.asarray(cols, dtype=np.int32)
    ne = int(cc.size)
    d = blocks["d"].astype(np.int64)
    cov_count = max(int((blocks["cov_off"].astype(np.int64) + d * d).max()), 1)
    blocks = np.ascontiguousarray(blocks)
    with torch.cuda.device(device):
        dev = _upload_named(device, blocks=_table_bytes(blocks), cols=cc, circular=_flags(circular))
        w_d = _f64(weights, device)
        mean = torch.empty(ne, dtype=torch.float64, device=device)
        res = torch.empty(ne, dtype=torch.float64, device=device)
        cov = torch.full((cov_count,), float("nan"), dtype=torch.float64, device=device)
        _check(lib().nfisam_sample_moments(_ptr(Xt), x_rows, n, blocks.ctypes.data_as(C.c_void_p), _ptr(dev["blocks"]), nb,
                                           _ptr(dev["cols"]), ne, _ptr(dev["circular"]), _ptr(w_d), _ptr(mean), _ptr(res),
                                           _ptr(cov), C.c_longlong(cov_count), _stream()), "nfisam_sample_moments")
    return mean, res, cov


def _check_probs(probs):
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 1 or p.size < 1:
        raise ValueError("probs must be a 1-D list of at least one probability")
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("a probability is outside [0, 1]: %s" % p[~((p >= 0.0) & (p <= 1.0))][:4])
    return np.ascontiguousarray(p)


def sample_quantiles(X, cols, probs, circular=None, center=None, device=None):
    """Quantiles at `probs` of the columns `cols` of X [n, x_cols] (tensor or numpy; float64 keys from float32 points):
    nfisam_sample_quantiles, one workgroup per column sorting in LDS, numpy's "linear" rule.  circular [n_entries] marks
    angles: their keys are wrap_pi(x - center[e]) (center [n_entries] float64, tensor or numpy: the circular means; None: 0)
    and center + quantile is returned UNWRAPPED -- wrap it for display.  n <= 16384.  -> [n_entries, n_probs] float64 device
    tensor."""
    device = _row_major_front("sample_quantiles", device, X=X)
    circular, center = _entry_arrays(circular, center)
    _check_quantile_args(int(X.shape[0]), int(X.shape[1]), cols, probs, circular, center)
    return sample_quantiles_t(_columns(X, device), cols, probs, circular, center, checked=True)


def _entry_arrays(circular, center):
    if circular is not None:
        circular = circular.detach().cpu().numpy() if torch.is_tensor(circular) else np.asarray(circular)
    if center is not None and not torch.is_tensor(center):
        center = np.asarray(center, dtype=np.float64)
    return circular, center


def _check_quantile_args(n, x_rows, cols, probs, circular, center):
    cols = np.asarray(cols)
    if cols.ndim != 1 or cols.size < 1:
        raise ValueError("cols must be a 1-D list of at least one row")
    _check_rows({"cols": (cols, x_rows)})
    _check_probs(probs)
    if not 1 <= n <= QUANTILE_MAX_N:
        raise ValueError("sample_quantiles takes 1..%d points, got %d" % (QUANTILE_MAX_N, n))
    for name, a in (("circular", circular), ("center", center)):
        if a is not None and (a.ndim != 1 or int(a.shape[0]) != cols.size):
            raise ValueError("%s must have one value per entry (%d)" % (name, cols.size))


def sample_quantiles_t(Xt, cols, probs, circular=None, center=None, checked=False):
    """`sample_quantiles` on the COLUMN-major matrix Xt [x_rows, n] (a contiguous float32 device tensor, used in place)."""
    x_rows, n = _column_major_front("Xt", Xt)
    device = Xt.device
    circular, center = _entry_arrays(circular, center)
    if not checked:
        _check_quantile_args(n, x_rows, cols, probs, circular, center)
    p = _check_probs(probs)
    cc = np.asarray(cols, dtype=np.int32)
    with torch.cuda.device(device):
        dev = _upload_named(device, cols=cc, probs=p, circular=_flags(circular), center=_entry_f64(center))
        out = torch.empty(int(cc.size), int(p.size), dtype=torch.float64, device=device)
        _check(lib().nfisam_sample_quantiles(_ptr(Xt), x_rows, n, _ptr(dev["cols"]), int(cc.size), _ptr(dev["circular"]),
                                             _ptr(dev["center"]), p.ctypes.data_as(C.c_void_p), _ptr(dev["probs"]), int(p.size),
                                             _ptr(out), _stream()), "nfisam_sample_quantiles")
    return out


# ---- posterior modes: mean-shift over every block's samples, then a merge (nfisam_sample_modes) ---------------------------------
MODE_KEYS = ("pos", "dens", "iters", "labels", "n_modes", "mode_pos", "mode_dens", "mode_mass", "unlabelled")


def check_mode_blocks(blocks: np.ndarray, cols, x_rows: int, scale=None, wrap=None) -> None:
    """ValueError for tables the kernels must not see: no block or more than 65535, d outside 1..16, a bandwidth term that is
    not positive and finite, entries outside [0, n_entries), two blocks that share an entry (the converged points are stored
    by entry: list a column twice instead), a row outside [0, x_rows), per-entry arrays of another length, a scale that is
    negative or not finite (a device tensor's length alone is checked: checking its values would read it back)."""
    cols = {"cols": (cols, x_rows)}
    off, d = _check_table_layout(blocks, MMD_BLOCK_DTYPE, "MMD_BLOCK_DTYPE", cols, dict(scale=scale, wrap=wrap), MODES_MAX_D)
    _check_disjoint(off, d, "the converged points are stored by entry (list the column twice)")
    _check_bandwidths(blocks)
    _check_rows(cols)
    if scale is not None and not (torch.is_tensor(scale) and scale.is_cuda):     # (a device tensor is taken as it is)
        sc = np.asarray(scale, dtype=np.float64)
        if not np.all(np.isfinite(sc)) or np.any(sc < 0):
            raise ValueError("scale must be finite and non-negative")


def check_mode_args(max_iters, tol, merge, max_modes) -> None:
    """ValueError for the scalar arguments nfisam_sample_modes refuses."""
    if int(max_iters) != max_iters or int(max_iters) < 1:
        raise ValueError("max_iters must be an integer >= 1, got %r" % (max_iters,))
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("tol must be finite and >= 0 (in sigmas), got %r" % (tol,))
    if not (np.isfinite(merge) and merge > 0):
        raise ValueError("merge must be finite and > 0 (in sigmas), got %r" % (merge,))
    if int(max_modes) != max_modes or not 1 <= int(max_modes) <= MODES_MAX_MODES:
        raise ValueError("max_modes must be an integer in 1..%d, got %r" % (MODES_MAX_MODES, max_modes))


def sample_modes(X, blocks: np.ndarray, cols, scale=None, wrap=None, weights=None, tol=1e-7, merge=1e-2, max_iters=500,
                 max_modes=16, device=None):
    """The modes of every block of `blocks` over the n rows of X [n, x_cols] (tensor or numpy; float32 points, float64
    arithmetic): nfisam_sample_modes -- a mean-shift ascent on the block's Gaussian kernel density estimate from every point,
    all iterations in one launch, and a deterministic merge of the converged points in a second.  `blocks`: numpy
    MMD_BLOCK_DTYPE (`pack_mmd_blocks`: widths 1..16 and the bandwidths sigma); entry e is column cols[e] of X; scale
    [n_entries] >= 0 multiplies an entry's differences in distances (0: the column is ignored there and carried along), wrap
    [n_entries] marks angles; weights [n] float64 (None: all ones); tol and merge in sigmas.  merge should stay well above
    tol * r / (1 - r), r the contraction per iteration of the slowest ascent (1e-5 sigma at tol = 1e-7 on a flat density):
    members of one mode end that far apart, and a smaller radius splits it.
    -> dict of device tensors: pos [n_entries, n] (converged points), dens [n_blocks, n], iters [n_blocks, n] int32 (negative:
    stopped on max_iters), labels [n_blocks, n] int32 (-1: left over), n_modes [n_blocks], mode_pos [n_blocks, max_modes, 16],
    mode_dens, mode_mass [n_blocks, max_modes] (NaN past n_modes), unlabelled [n_blocks]."""
    device = _row_major_front("sample_modes", device, X=X)
    if int(X.shape[0]) < 1:
        raise ValueError("sample_modes: no points")
    check_mode_blocks(blocks, cols, int(X.shape[1]), scale, wrap)
    check_mode_args(max_iters, tol, merge, max_modes)
    weights = _check_weights(weights, int(X.shape[0]))
    return sample_modes_t(_columns(X, device), blocks, cols, scale, wrap, weights, tol, merge, max_iters, max_modes, checked=True)


def _mode_shapes(blocks, cols, n, max_modes):
    """{key of MODE_KEYS: (shape, dtype)} of the tensors of a modes call."""
    nb, ne, mm = int(blocks.shape[0]), int(np.size(cols)), max(int(max_modes), 1)
    return dict(pos=((ne, n), torch.float64), dens=((nb, n), torch.float64), iters=((nb, n), torch.int32),
                labels=((nb, n), torch.int32), n_modes=((nb,), torch.int32), mode_pos=((nb, mm, MODES_MAX_D), torch.float64),
                mode_dens=((nb, mm), torch.float64), mode_mass=((nb, mm), torch.float64), unlabelled=((nb,), torch.int32))


def _modes_inputs(device, blocks, cols, scale, wrap, weights, shapes, given):
    """What sample_modes_t and sample_modes_merge_t share once their arguments are checked
    -> (the contiguous host table, the tables and per-entry arrays on the device by name (one upload), the weights on the
    device or None, the result dict: the tensors `given` as they are, the others of `shapes` fresh)."""
    blocks = np.ascontiguousarray(blocks)
    dev = _upload_named(device, blocks=_table_bytes(blocks), cols=np.asarray(cols, dtype=np.int32), scale=_entry_f64(scale),
                        wrap=_flags(wrap))
    res = {k: given[k] if k in given else torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in shapes.items()}
    return blocks, dev, _f64(weights, device), res


def sample_modes_t(Xt, blocks: np.ndarray, cols, scale=None, wrap=None, weights=None, tol=1e-7, merge=1e-2, max_iters=500,
                   max_modes=16, checked=False, out=None):
    """`sample_modes` on the COLUMN-major matrix Xt [x_rows, n] (a contiguous float32 device tensor, used in place): what the
    tree walk wrote.  `checked` skips the table and argument checks (the caller has made them); `out`: the dict of an earlier
    call with the same shapes, written in place."""
    x_rows, n = _column_major_front("Xt", Xt)
    if n < 1:
        raise ValueError("sample_modes: no points")
    if not checked:
        check_mode_blocks(blocks, cols, x_rows, scale, wrap)
        check_mode_args(max_iters, tol, merge, max_modes)
        weights = _check_weights(weights, n)
    device, shapes = Xt.device, _mode_shapes(blocks, cols, n, max_modes)
    if out is not None:
        for k, (shape, dt) in shapes.items():
            t = out.get(k)
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != device or not t.is_contiguous():
                raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s" % (k, dt, shape, device))
    with torch.cuda.device(device):
        blocks, dev, w_d, res = _modes_inputs(device, blocks, cols, scale, wrap, weights, shapes, out or {})
        _check(lib().nfisam_sample_modes(_ptr(Xt), x_rows, n, blocks.ctypes.data_as(C.c_void_p), _ptr(dev["blocks"]),
                                         int(blocks.shape[0]), _ptr(dev["cols"]), shapes["pos"][0][0], _ptr(dev["scale"]),
                                         _ptr(dev["wrap"]), _ptr(w_d), C.c_int(int(max_iters)), C.c_double(float(tol)),
                                         C.c_double(float(merge)), C.c_int(int(max_modes)), *[_ptr(res[k]) for k in MODE_KEYS],
                                         _stream()), "nfisam_sample_modes")
    return res if out is None else out


def sample_modes_merge_t(out, x_rows: int, blocks: np.ndarray, cols, scale=None, wrap=None, weights=None, merge=1e-2, max_modes=16,
                         checked=False):
    """The merge alone (nfisam_sample_modes_merge): the converged points `out["pos"]` and densities `out["dens"]` of an earlier
    `sample_modes` / `sample_modes_t` call -- same table, cols, scale, wrap, weights -- merged again with another radius or
    max_modes, without climbing again.  x_rows: the rows of the matrix the call was made on.  -> a new dict that shares pos,
    dens and iters with `out`; the same bits as a full call with these arguments."""
    for k in MODE_KEYS[:3]:
        t = out.get(k) if isinstance(out, dict) else None
        if not torch.is_tensor(t) or not t.is_cuda or t.ndim != 2 or not t.is_contiguous():
            raise ValueError("out[%r] must be the contiguous device tensor of an earlier sample_modes call" % k)
    pos, dens = out["pos"], out["dens"]
    n = int(pos.shape[1])
    if not checked:
        check_mode_blocks(blocks, cols, x_rows, scale, wrap)
        check_mode_args(1, 0.0, merge, max_modes)
        weights = _check_weights(weights, n)
    shapes = _mode_shapes(blocks, cols, n, max_modes)
    if n < 1 or any((tuple(t.shape), t.dtype) != shapes[k] for k, t in (("pos", pos), ("dens", dens))):
        raise ValueError("out does not belong to this table: pos %s, dens %s for %d entries, %d blocks" %
                         (tuple(pos.shape), tuple(dens.shape), shapes["pos"][0][0], shapes["dens"][0][0]))
    with torch.cuda.device(pos.device):
        blocks, dev, w_d, res = _modes_inputs(pos.device, blocks, cols, scale, wrap, weights, shapes,
                                              {k: out[k] for k in MODE_KEYS[:3]})
        _check(lib().nfisam_sample_modes_merge(int(x_rows), n, blocks.ctypes.data_as(C.c_void_p), _ptr(dev["blocks"]),
                                               int(blocks.shape[0]), _ptr(dev["cols"]), shapes["pos"][0][0], _ptr(dev["scale"]),
                                               _ptr(dev["wrap"]), _ptr(w_d), C.c_double(float(merge)), C.c_int(int(max_modes)),
                                               _ptr(pos), _ptr(dens), *[_ptr(res[k]) for k in MODE_KEYS[3:]], _stream()),
               "nfisam_sample_modes_merge")
    return res


# ---- k nearest neighbours and ball counts: a selection over pairs (nfisam_sample_knn, nfisam_sample_ball_count) ---------------
class KnnBlock(C.Structure):
    _fields_ = [("col_off", C.c_int32), ("d", C.c_int32), ("radius_row", C.c_int32), ("reserved", C.c_int32)]


KNN_BLOCK_DTYPE = np.dtype([("col_off", np.int32), ("d", np.int32), ("radius_row", np.int32), ("reserved", np.int32)])
assert KNN_BLOCK_DTYPE.itemsize == C.sizeof(KnnBlock) == 16
KNN_MAX_D, KNN_MAX_K = 16, 16                    # NFISAM_KNN_MAX_D, NFISAM_KNN_MAX_K
KNN_NORMS = {"max": 0, "l2": 1}                  # NFISAM_KNN_NORM_MAX, NFISAM_KNN_NORM_L2
KNN_KEYS = ("dist", "idx", "log_sum", "n_used")


def pack_knn_blocks(dims, radius_rows=None) -> np.ndarray:
    """The block table (numpy KNN_BLOCK_DTYPE) of consecutive blocks of `dims` entries; radius_rows: the row of `radius` each
    block's queries take in `sample_ball_count` (default: all 0)."""
    dims, t = _consecutive(dims, KNN_BLOCK_DTYPE)
    if radius_rows is not None:
        t["radius_row"] = np.asarray(radius_rows, dtype=np.int64).reshape(-1)
    return t


def check_knn_blocks(blocks: np.ndarray, xcols, ycols, x_rows: int, y_rows: int, scale=None, wrap=None, n_radius: int = None) -> None:
    """ValueError for tables the kernels must not see: no block or more than 65535, d outside 1..16, entries outside
    [0, n_entries), a row outside [0, x_rows) / [0, y_rows), per-entry arrays of another length, a scale that is not finite
    (a device tensor's length alone is checked), with `n_radius` a radius_row outside [0, n_radius)."""
    cols = {"xcols": (xcols, x_rows), "ycols": (ycols, y_rows)}
    _check_table_layout(blocks, KNN_BLOCK_DTYPE, "KNN_BLOCK_DTYPE", cols, dict(scale=scale, wrap=wrap), KNN_MAX_D)
    _check_rows(cols)
    if not (torch.is_tensor(scale) and scale.is_cuda):                            # (a device tensor is taken as it is)
        _check_finite("scale", scale)
    if n_radius is not None:
        rr = blocks["radius_row"].astype(np.int64)
        bad = (rr < 0) | (rr >= int(n_radius))
        if np.any(bad):
            b = int(np.argmax(bad))
            raise ValueError("block %d: radius_row %d is out of range of the %d rows of radius" % (b, int(rr[b]), int(n_radius)))


def check_knn_args(m: int, n: int, k=1, norm="max", exclude_self=False) -> int:
    """ValueError for the scalar arguments nfisam_sample_knn / nfisam_sample_ball_count refuse -> the norm's code."""
    if m < 1 or n < 1:
        raise ValueError("both sample sets need at least one point")
    if max(m, n) > 65535 * 64:
        raise ValueError("%d x %d points are out of range of the grid (65535 tiles of 64)" % (m, n))
    if int(k) != k or not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError("k must be an integer in 1..%d, got %r" % (KNN_MAX_K, k))
    if norm not in KNN_NORMS:
        raise ValueError("norm must be one of %s, got %r" % (sorted(KNN_NORMS), norm))
    if exclude_self and m != n:
        raise ValueError("exclude_self needs the two sets to be one (m = %d, n = %d)" % (m, n))
    return KNN_NORMS[norm]


def sample_knn(X, Y, blocks: np.ndarray, xcols, ycols, k=4, norm="max", scale=None, wrap=None, exclude_self=False, device=None):
    """The k nearest neighbours of every row of X [m, x_cols] among the rows of Y [n, y_cols] (tensor or numpy; Y None: X
    itself), within every block of `blocks`: nfisam_sample_knn, all blocks in one launch on the current stream.  `blocks`:
    numpy KNN_BLOCK_DTYPE (`pack_knn_blocks`: widths 1..16); entry e of a block pairs column xcols[e] of X with column
    ycols[e] of Y; scale [n_entries] multiplies an entry's differences, wrap [n_entries] marks angles (differences brought
    into [-pi, pi)); norm "max" or "l2"; exclude_self skips the pair j == i (m == n).
    -> dict of device tensors: dist [n_blocks, k, m] float64 ascending in k (+inf where there is no candidate), idx
    [n_blocks, k, m] int32 (-1 there; equal distances by ascending j), log_sum [n_blocks] float64 (the sum of log(k-th
    distance) over the queries where that is positive and finite), n_used [n_blocks] int32 (how many those were)."""
    mats = dict(X=X) if Y is None else dict(X=X, Y=Y)
    device = _row_major_front("sample_knn", device, **mats)
    other = X if Y is None else Y
    check_knn_blocks(blocks, xcols, ycols, int(X.shape[1]), int(other.shape[1]), scale, wrap)
    check_knn_args(int(X.shape[0]), int(other.shape[0]), k, norm, exclude_self)
    Xt = _columns(X, device)
    return sample_knn_t(Xt, None if Y is None else _columns(Y, device), blocks, xcols, ycols, k, norm, scale, wrap, exclude_self,
                        checked=True)


def sample_knn_t(Xt, Yt, blocks: np.ndarray, xcols, ycols, k=4, norm="max", scale=None, wrap=None, exclude_self=False,
                 checked=False, out=None):
    """`sample_knn` on the COLUMN-major matrices Xt [x_rows, m], Yt [y_rows, n] (contiguous float32 device tensors, used in
    place; Yt None: Xt): what the tree walk wrote.  `checked` skips the table and argument checks (the caller has made them);
    `out`: the dict of an earlier call with the same shapes, written in place."""
    Yt, x_rows, m, y_rows, n = _two_set_front(("Xt", "Yt"), Xt, Yt, same=True)
    if not checked:
        check_knn_blocks(blocks, xcols, ycols, x_rows, y_rows, scale, wrap)
        check_knn_args(m, n, k, norm, exclude_self)
    device, nb, kk = Xt.device, int(blocks.shape[0]), max(int(k), 1)
    shapes = dict(dist=((nb, kk, m), torch.float64), idx=((nb, kk, m), torch.int32), log_sum=((nb,), torch.float64),
                  n_used=((nb,), torch.int32))
    if out is not None:
        for key, (shape, dt) in shapes.items():
            t = out.get(key)
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != device or not t.is_contiguous():
                raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s" % (key, dt, shape, device))
    blocks = np.ascontiguousarray(blocks)
    with torch.cuda.device(device):
        dev, ne = _two_set_upload(device, blocks, ("xcols", "ycols"), xcols, ycols, scale=_entry_f64(scale), wrap=_flags(wrap))
        res = out if out is not None else {key: torch.empty(shape, dtype=dt, device=device) for key, (shape, dt) in shapes.items()}
        _check(lib().nfisam_sample_knn(_ptr(Xt), x_rows, m, _ptr(Yt), y_rows, n, C.c_int(1 if exclude_self else 0),
                                       blocks.ctypes.data_as(C.c_void_p), _ptr(dev["blocks"]), nb, _ptr(dev["xcols"]),
                                       _ptr(dev["ycols"]), ne, _ptr(dev["scale"]), _ptr(dev["wrap"]), C.c_int(int(k)),
                                       C.c_int(KNN_NORMS.get(norm, -1) if isinstance(norm, str) else int(norm)),
                                       *[_ptr(res[key]) for key in KNN_KEYS], _stream()), "nfisam_sample_knn")
    return res


def sample_ball_count(X, Y, blocks: np.ndarray, xcols, ycols, radius, norm="max", scale=None, wrap=None, exclude_self=False,
                      device=None):
    """How many rows of Y [n, y_cols] (None: X itself) lie STRICTLY inside a radius of every row of X [m, x_cols], within every
    block of `blocks`: nfisam_sample_ball_count, all blocks in one launch.  radius [n_radius, m] float64 (tensor or numpy):
    block b's query i takes radius[blocks["radius_row"][b], i]; a NaN or negative radius counts nothing.  The other arguments
    are those of `sample_knn`.  -> count [n_blocks, m] int32 device tensor."""
    mats = dict(X=X) if Y is None else dict(X=X, Y=Y)
    device = _row_major_front("sample_ball_count", device, **mats)
    other = X if Y is None else Y
    m = int(X.shape[0])
    if not (torch.is_tensor(radius) or isinstance(radius, np.ndarray)) or radius.ndim != 2 or int(radius.shape[1]) != m or \
            int(radius.shape[0]) < 1:
        raise ValueError("radius must be [n_radius, m] = [>= 1, %d]" % m)
    check_knn_blocks(blocks, xcols, ycols, int(X.shape[1]), int(other.shape[1]), scale, wrap, int(radius.shape[0]))
    check_knn_args(m, int(other.shape[0]), 1, norm, exclude_self)
    Xt = _columns(X, device)
    return sample_ball_count_t(Xt, None if Y is None else _columns(Y, device), blocks, xcols, ycols, _f64(radius, device), norm,
                               scale, wrap, exclude_self, checked=True)


def sample_ball_count_t(Xt, Yt, blocks: np.ndarray, xcols, ycols, radius, norm="max", scale=None, wrap=None, exclude_self=False,
                        checked=False, out=None):
    """`sample_ball_count` on the COLUMN-major matrices Xt [x_rows, m], Yt [y_rows, n] (Yt None: Xt); radius: a contiguous
    float64 [n_radius, m] tensor on their device (rows of a `sample_knn_t` result's dist, for instance).  `out`: an int32
    [n_blocks, m] device tensor written in place."""
    Yt, x_rows, m, y_rows, n = _two_set_front(("Xt", "Yt"), Xt, Yt, same=True)
    if not torch.is_tensor(radius) or not radius.is_cuda:
        raise RuntimeError("radius must be a tensor on a ROCm device (no CPU path exists)")
    if radius.ndim != 2 or radius.dtype != torch.float64 or not radius.is_contiguous() or int(radius.shape[1]) != m or \
            int(radius.shape[0]) < 1 or radius.device != Xt.device:
        raise ValueError("radius must be a contiguous float64 [n_radius, m] = [>= 1, %d] tensor on %s" % (m, Xt.device))
    n_radius = int(radius.shape[0])
    if not checked:
        check_knn_blocks(blocks, xcols, ycols, x_rows, y_rows, scale, wrap, n_radius)
        check_knn_args(m, n, 1, norm, exclude_self)
    device, nb = Xt.device, int(blocks.shape[0])
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != (nb, m) or out.dtype != torch.int32 or
                            out.device != device or not out.is_contiguous()):
        raise ValueError("out must be a contiguous int32 tensor of shape %s on %s" % ((nb, m), device))
    blocks = np.ascontiguousarray(blocks)
    with torch.cuda.device(device):
        dev, ne = _two_set_upload(device, blocks, ("xcols", "ycols"), xcols, ycols, scale=_entry_f64(scale), wrap=_flags(wrap))
        count = out if out is not None else torch.empty(nb, m, dtype=torch.int32, device=device)
        _check(lib().nfisam_sample_ball_count(_ptr(Xt), x_rows, m, _ptr(Yt), y_rows, n, C.c_int(1 if exclude_self else 0),
                                              blocks.ctypes.data_as(C.c_void_p), _ptr(dev["blocks"]), nb, _ptr(dev["xcols"]),
                                              _ptr(dev["ycols"]), ne, _ptr(dev["scale"]), _ptr(dev["wrap"]),
                                              C.c_int(KNN_NORMS.get(norm, -1) if isinstance(norm, str) else int(norm)),
                                              _ptr(radius), n_radius, _ptr(count), _stream()), "nfisam_sample_ball_count")
    return count


# ---- marginal densities at query points: a Gaussian kernel density estimate in logs (nfisam_sample_density) --------------------
class DensityBlock(C.Structure):
    _fields_ = [("col_off", C.c_int32), ("d", C.c_int32), ("log_norm", C.c_double), ("whiten", C.c_double * 21)]


DENSITY_BLOCK_DTYPE = np.dtype([("col_off", np.int32), ("d", np.int32), ("log_norm", np.float64), ("whiten", np.float64, (21,))])
assert DENSITY_BLOCK_DTYPE.itemsize == C.sizeof(DensityBlock) == 184
DENSITY_MAX_D = 6                                # NFISAM_DENSITY_MAX_D
DENSITY_MAX_WIDTH = np.pi / 3.0                  # widest kernel on a circular entry: the nearest image alone is summed
_TRIL = [np.tril_indices(d) for d in range(DENSITY_MAX_D + 1)]


def pack_density_blocks(dims, whiten, col_off=None) -> np.ndarray:
    """The block table (numpy DENSITY_BLOCK_DTYPE) of blocks of `dims` entries; whiten[b]: block b's lower-triangular [d, d]
    matrix W with W H W' = I for its bandwidth matrix H (inv(cholesky(H)); the upper triangle is not read); log_norm =
    sum_r log W_rr - d/2 log(2 pi) is formed here.  col_off: each block's first entry (default: consecutive blocks) -- blocks
    may share entries, which is how bandwidth candidates of one column set go into one launch."""
    dims, t = _consecutive(dims, DENSITY_BLOCK_DTYPE)
    if len(whiten) != dims.size:
        raise ValueError("one whitening matrix per block (%d), got %d" % (dims.size, len(whiten)))
    if col_off is not None:
        t["col_off"] = np.asarray(col_off, dtype=np.int64).reshape(-1)
    for b, (d, W) in enumerate(zip(dims, whiten)):
        W = np.asarray(W, dtype=np.float64)
        if not 1 <= d <= DENSITY_MAX_D or W.shape != (d, d):
            raise ValueError("block %d: a whitening matrix is [d, d] with d in 1..%d, got d = %d and shape %s"
                             % (b, DENSITY_MAX_D, d, W.shape))
        t["whiten"][b, :d * (d + 1) // 2] = W[_TRIL[d]]
        with np.errstate(divide="ignore", invalid="ignore"):
            t["log_norm"][b] = np.log(np.diag(W)).sum() - 0.5 * d * np.log(2.0 * np.pi)
    return t


def check_density_blocks(blocks: np.ndarray, qcols, xcols, q_rows: int, x_rows: int, wrap=None) -> None:
    """ValueError for tables the kernel must not see: no block or more than 65535, d outside 1..6, entries outside
    [0, n_entries), a row outside [0, q_rows) / [0, x_rows), flags of another length, a log_norm or whitening entry that is
    not finite, a diagonal entry <= 0, and a circular entry whose kernel width 1 / W_rr exceeds pi / 3."""
    cols = {"qcols": (qcols, q_rows), "xcols": (xcols, x_rows)}
    off, d = _check_table_layout(blocks, DENSITY_BLOCK_DTYPE, "DENSITY_BLOCK_DTYPE", cols, dict(wrap=wrap), DENSITY_MAX_D)
    _check_rows(cols)
    flags = None if wrap is None else np.asarray(wrap).astype(bool)
    for b in range(blocks.size):
        k = int(d[b])
        tri = blocks["whiten"][b, :k * (k + 1) // 2]
        diag = tri[np.cumsum(np.arange(1, k + 1)) - 1]
        if not np.isfinite(blocks["log_norm"][b]) or not np.all(np.isfinite(tri)):
            raise ValueError("block %d: log_norm and the whitening matrix must be finite" % b)
        if not np.all(diag > 0):
            raise ValueError("block %d: the whitening matrix needs a positive diagonal" % b)
        if flags is not None:
            wide = flags[off[b]:off[b] + k] & (1.0 / diag > DENSITY_MAX_WIDTH)
            if np.any(wide):
                r = int(np.argmax(wide))
                raise ValueError("block %d: the kernel of circular entry %d is %.3g rad wide; beyond pi / 3 the nearest image "
                                 "alone no longer carries its mass" % (b, r, 1.0 / diag[r]))


def check_density_args(m: int, n: int, exclude_self=False) -> None:
    """ValueError for the scalar arguments nfisam_sample_density refuses."""
    if m < 1 or n < 1:
        raise ValueError("queries and samples need at least one point each")
    if m > 65535 * 64:
        raise ValueError("%d queries are out of range of the grid (65535 tiles of 64)" % m)
    if exclude_self and m != n:
        raise ValueError("exclude_self needs the queries to be the samples (m = %d, n = %d)" % (m, n))


def density_log_weights(weights, n: int, device, checked=False):
    """Checked weights (None, numpy or a device tensor) -> (log_w float64 [n] on `device` with -inf for a zero weight, log of
    their sum); (None, 0.0) without weights.  The logs are formed on the device."""
    if not checked:
        weights = _check_weights(weights, n)
    if weights is None:
        return None, 0.0
    w = _f64(weights, device)
    return torch.log(w), float(torch.log(w.sum()).item())


def sample_density(q, x, blocks: np.ndarray, qcols, xcols, wrap=None, weights=None, exclude_self=False, want_density=False,
                   device=None):
    """The Gaussian kernel density estimate of the rows of x [n, x_cols] (tensor or numpy; None: q itself) at the rows of q
    [m, q_cols], within every block of `blocks`, in logs: nfisam_sample_density, all blocks in one launch on the current
    stream.  `blocks`: numpy DENSITY_BLOCK_DTYPE (`pack_density_blocks`: widths 1..6, a whitening matrix each); entry e of a
    block pairs column qcols[e] of q with column xcols[e] of x; wrap [n_entries] marks angles (differences brought into
    [-pi, pi), the nearest image alone); weights [n]: non-negative, None for all ones; exclude_self skips the pair j == i
    (m == n): the leave-one-out density.
    -> dict of device tensors: log_density [n_blocks, m] float64, density (the same shape with want_density, else None)."""
    mats = dict(q=q) if x is None else dict(q=q, x=x)
    device = _row_major_front("sample_density", device, **mats)
    other = q if x is None else x
    check_density_blocks(blocks, qcols, xcols, int(q.shape[1]), int(other.shape[1]), wrap)
    check_density_args(int(q.shape[0]), int(other.shape[0]), exclude_self)
    weights = _check_weights(weights, int(other.shape[0]))
    Qt = _columns(q, device)
    return sample_density_t(Qt, None if x is None else _columns(x, device), blocks, qcols, xcols, wrap, None, exclude_self,
                            want_density, checked=True, weights=weights)


def sample_density_t(Qt, Xt, blocks: np.ndarray, qcols, xcols, wrap=None, log_w=None, exclude_self=False, want_density=False,
                     checked=False, weights=None, log_w_sum=None):
    """`sample_density` on the COLUMN-major matrices Qt [q_rows, m], Xt [x_rows, n] (contiguous float32 device tensors, used
    in place; Xt None: Qt): what the tree walk wrote.  log_w: None or a float64 [n] tensor on their device (-inf: a zero
    weight) with log_w_sum the log of the weights' sum (None: formed on the device); or `weights`, from which both are formed
    on the device (`density_log_weights`).  `checked` skips the table, argument and weight checks (the caller has made them)."""
    Xt, q_rows, m, x_rows, n = _two_set_front(("Qt", "Xt"), Qt, Xt, same=True)
    device = Qt.device
    if log_w is not None and weights is not None:
        raise ValueError("give log_w or weights, not both")
    if log_w is not None and (not torch.is_tensor(log_w) or log_w.dtype != torch.float64 or tuple(log_w.shape) != (n,) or
                              log_w.device != device or not log_w.is_contiguous()):
        raise ValueError("log_w must be a contiguous float64 [n] = [%d] tensor on %s" % (n, device))
    if not checked:
        check_density_blocks(blocks, qcols, xcols, q_rows, x_rows, wrap)
        check_density_args(m, n, exclude_self)
        weights = _check_weights(weights, n)
    nb = int(blocks.shape[0])
    blocks = np.ascontiguousarray(blocks)
    with torch.cuda.device(device):
        dev, ne = _two_set_upload(device, blocks, ("qcols", "xcols"), qcols, xcols, wrap=_flags(wrap))
        if weights is not None:
            log_w, log_w_sum = density_log_weights(weights, n, device, checked=True)
        elif log_w is not None and log_w_sum is None:
            log_w_sum = float(torch.logsumexp(log_w, 0).item())
        log_dens = torch.empty(nb, m, dtype=torch.float64, device=device)
        dens = torch.empty(nb, m, dtype=torch.float64, device=device) if want_density else None
        _check(lib().nfisam_sample_density(_ptr(Qt), q_rows, m, _ptr(Xt), x_rows, n, C.c_int(1 if exclude_self else 0),
                                           blocks.ctypes.data_as(C.c_void_p), _ptr(dev["blocks"]), nb, _ptr(dev["qcols"]),
                                           _ptr(dev["xcols"]), ne, _ptr(dev["wrap"]), _ptr(log_w),
                                           C.c_double(0.0 if log_w_sum is None else log_w_sum), _ptr(log_dens), _ptr(dens),
                                           _stream()), "nfisam_sample_density")
    return dict(log_density=log_dens, density=dens)


# ---- trajectory error per sample: aligned ATE and RPE (nfisam_sample_trajectory_error, nfisam_sample_trajectory_rpe) ------------
class TrajEntry(C.Structure):
    _fields_ = [("col_x", C.c_int32), ("col_y", C.c_int32), ("col_th", C.c_int32), ("flags", C.c_int32), ("ax", C.c_double),
                ("ay", C.c_double), ("ath", C.c_double)]


class TrajPair(C.Structure):
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("slot", C.c_int32), ("reserved", C.c_int32)]


TRAJ_ENTRY_DTYPE = np.dtype([("col_x", np.int32), ("col_y", np.int32), ("col_th", np.int32), ("flags", np.int32),
                             ("ax", np.float64), ("ay", np.float64), ("ath", np.float64)])
TRAJ_PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("slot", np.int32), ("reserved", np.int32)])
assert TRAJ_ENTRY_DTYPE.itemsize == C.sizeof(TrajEntry) == 40 and TRAJ_PAIR_DTYPE.itemsize == C.sizeof(TrajPair) == 16
TRAJ_ALIGNED, TRAJ_LANDMARK = 1, 2                # NFISAM_TRAJ_ALIGNED, NFISAM_TRAJ_LANDMARK
TRAJ_MODES = {"none": 0, "rigid": 1, "similarity": 2}                 # NFISAM_TRAJ_ALIGN_*
TRAJ_OUT_ROWS = 8                                 # NFISAM_TRAJ_OUT_ROWS
TRAJ_ERROR_KEYS = ("theta", "scale", "t", "sse_traj", "sse_landmark", "sse_heading", "worst", "reflected", "worst_entry",
                   "entry_sums", "weight_sum", "n_traj", "n_landmark", "n_heading")


def pack_traj_entries(col_x, col_y, col_th, truth_xy, truth_th=None, aligned=None, landmark=None) -> np.ndarray:
    """The entry table (numpy TRAJ_ENTRY_DTYPE): entry e reads the rows col_x[e], col_y[e] and col_th[e] (-1: no heading) of
    the column-major matrix and is graded against truth_xy[e] (and truth_th[e]).  aligned [P] (default: every entry that is no
    landmark) marks the entries of the alignment, landmark [P] (default: none) those whose residual goes to the landmark sum."""
    col_x = np.asarray(col_x, dtype=np.int64).reshape(-1)
    P = col_x.size
    xy = np.asarray(truth_xy, dtype=np.float64).reshape(-1, 2) if P else np.zeros((0, 2))
    th = np.zeros(P) if truth_th is None else np.asarray(truth_th, dtype=np.float64).reshape(-1)
    land = np.zeros(P, dtype=bool) if landmark is None else np.asarray(landmark, dtype=bool).reshape(-1)
    al = ~land if aligned is None else np.asarray(aligned, dtype=bool).reshape(-1)
    col_y, col_th = np.asarray(col_y, dtype=np.int64).reshape(-1), np.asarray(col_th, dtype=np.int64).reshape(-1)
    if not (col_y.size == col_th.size == th.size == land.size == al.size == xy.shape[0] == P):
        raise ValueError("pack_traj_entries: one row triple, one truth and one flag per entry (%d)" % P)
    t = np.zeros(P, dtype=TRAJ_ENTRY_DTYPE)
    t["col_x"], t["col_y"], t["col_th"] = col_x, col_y, col_th
    t["flags"] = al.astype(np.int32) * TRAJ_ALIGNED + land.astype(np.int32) * TRAJ_LANDMARK
    t["ax"], t["ay"], t["ath"] = xy[:, 0], xy[:, 1], np.where(col_th >= 0, th, 0.0)
    return t


def pack_traj_pairs(poses, strides) -> np.ndarray:
    """The pair table (numpy TRAJ_PAIR_DTYPE) of a time-ordered list `poses` of entries: slot s holds the pairs
    (poses[k], poses[k + strides[s]])."""
    poses = np.asarray(poses, dtype=np.int64).reshape(-1)
    rows = []
    for s, k in enumerate(strides):
        k = int(k)
        if not 1 <= k < poses.size:
            raise ValueError("pack_traj_pairs: stride %d needs 1 <= stride < %d poses" % (k, poses.size))
        rows.extend((int(a), int(b), s, 0) for a, b in zip(poses[:-k], poses[k:]))
    if not rows:
        raise ValueError("pack_traj_pairs: no stride")
    return np.array(rows, dtype=TRAJ_PAIR_DTYPE)


def check_traj_entries(entries: np.ndarray, x_rows: int, align="rigid") -> int:
    """ValueError for what the kernels must not see: a table of another dtype or without entries, a row outside [0, x_rows)
    (col_th: -1 or a row), an unknown flag, a truth that is not finite, an unknown mode, an aligned mode without an aligned
    entry.  -> the mode's number."""
    if align not in TRAJ_MODES:
        raise ValueError("align is one of %s, got %r" % (", ".join(repr(k) for k in TRAJ_MODES), align))
    if not isinstance(entries, np.ndarray) or entries.dtype != TRAJ_ENTRY_DTYPE or entries.ndim != 1:
        raise ValueError("entries must be a 1-D numpy array of TRAJ_ENTRY_DTYPE")
    if entries.size < 1:
        raise ValueError("entries: at least one entry is needed (P >= 1)")
    for name, low in (("col_x", 0), ("col_y", 0), ("col_th", -1)):
        c = entries[name]
        if int(c.min()) < low or int(c.max()) >= int(x_rows):
            raise ValueError("entry %d: %s = %d is out of range of the %d rows of the matrix"
                             % (int(np.argmax((c < low) | (c >= int(x_rows)))), name, int(c[np.argmax((c < low) | (c >= int(x_rows)))]),
                                int(x_rows)))
    if np.any(entries["flags"] & ~(TRAJ_ALIGNED | TRAJ_LANDMARK)):
        raise ValueError("entry %d: unknown flag" % int(np.argmax(entries["flags"] & ~(TRAJ_ALIGNED | TRAJ_LANDMARK) != 0)))
    ok = np.isfinite(entries["ax"]) & np.isfinite(entries["ay"]) & (np.isfinite(entries["ath"]) | (entries["col_th"] < 0))
    if not np.all(ok):
        raise ValueError("entry %d: the truth is not finite" % int(np.argmin(ok)))
    if align != "none" and not np.any(entries["flags"] & TRAJ_ALIGNED):
        raise ValueError("align=%r needs at least one aligned entry" % align)
    return TRAJ_MODES[align]


def check_traj_pairs(pairs: np.ndarray, entries: np.ndarray, n_slots: int = None) -> int:
    """ValueError for a pair table of another dtype or without pairs, a pair that names an entry outside the table or one
    without a heading, a slot outside [0, n_slots) (default: the largest slot + 1; at most 65535).  -> n_slots."""
    if not isinstance(pairs, np.ndarray) or pairs.dtype != TRAJ_PAIR_DTYPE or pairs.ndim != 1:
        raise ValueError("pairs must be a 1-D numpy array of TRAJ_PAIR_DTYPE")
    if pairs.size < 1:
        raise ValueError("pairs: at least one pair is needed")
    P = int(entries.size)
    for name in ("i", "j"):
        bad = (pairs[name] < 0) | (pairs[name] >= P)
        if np.any(bad):
            raise ValueError("pair %d: %s = %d is outside the %d entries" % (int(np.argmax(bad)), name, int(pairs[name][np.argmax(bad)]), P))
        blind = entries["col_th"][pairs[name]] < 0
        if np.any(blind):
            raise ValueError("pair %d: entry %d has no heading" % (int(np.argmax(blind)), int(pairs[name][np.argmax(blind)])))
    n_slots = int(pairs["slot"].max()) + 1 if n_slots is None else int(n_slots)
    if not 1 <= n_slots <= 65535:
        raise ValueError("1..65535 slots are supported, got %d" % n_slots)
    bad = (pairs["slot"] < 0) | (pairs["slot"] >= n_slots)
    if np.any(bad):
        raise ValueError("pair %d: slot %d is outside [0, %d)" % (int(np.argmax(bad)), int(pairs["slot"][np.argmax(bad)]), n_slots))
    return n_slots


def sample_trajectory_error(X, entries: np.ndarray, align="rigid", reflect=False, weights=None, device=None):
    """Every row of X [n, x_cols] (tensor or numpy; float32 points, float64 arithmetic) aligned to the ground truth of
    `entries` and graded: nfisam_sample_trajectory_error, one sample per lane, on the current stream.  `entries`: numpy
    TRAJ_ENTRY_DTYPE (`pack_traj_entries`), its rows naming COLUMNS of X; align "none", "rigid" (theta, t) or "similarity"
    (and the least-squares scale); reflect: also try the improper fit; weights [n] float64 (None: all ones) enter entry_sums
    alone.  -> dict: theta, scale, sse_traj, sse_landmark, sse_heading, worst [n] float64, t [2, n] float64, reflected,
    worst_entry [n] int32, entry_sums [P] float64 (sum_i w_i |r_e,i|^2), weight_sum (a 0-d tensor) -- on the device -- and the
    counts n_traj, n_landmark, n_heading of the table."""
    device = _row_major_front("sample_trajectory_error", device, X=X)
    if int(X.shape[0]) < 1:
        raise ValueError("sample_trajectory_error: no points")
    check_traj_entries(entries, int(X.shape[1]), align)
    weights = _check_weights(weights, int(X.shape[0]))
    return sample_trajectory_error_t(_columns(X, device), entries, align, reflect, weights, checked=True)


def sample_trajectory_error_t(Xt, entries: np.ndarray, align="rigid", reflect=False, weights=None, checked=False):
    """`sample_trajectory_error` on the COLUMN-major matrix Xt [x_rows, n] (a contiguous float32 device tensor, used in place):
    what the tree walk wrote.  `checked` skips the table and weight checks (the caller has made them)."""
    x_rows, n = _column_major_front("Xt", Xt)
    device = Xt.device
    if n < 1:
        raise ValueError("sample_trajectory_error: no points")
    if not checked:
        check_traj_entries(entries, x_rows, align)
        weights = _check_weights(weights, n)
    entries = np.ascontiguousarray(entries)
    P = int(entries.size)
    land = (entries["flags"] & TRAJ_LANDMARK) != 0
    with torch.cuda.device(device):
        dev = _upload_named(device, entries=_table_bytes(entries))
        w_d = _f64(weights, device)
        out = torch.empty(TRAJ_OUT_ROWS, n, dtype=torch.float64, device=device)
        iout = torch.empty(2, n, dtype=torch.int32, device=device)
        sums = torch.empty(P + 1, dtype=torch.float64, device=device)
        scratch = torch.empty(int(lib().nfisam_sample_trajectory_scratch_count(n, P)), dtype=torch.float64, device=device)
        _check(lib().nfisam_sample_trajectory_error(_ptr(Xt), x_rows, n, entries.ctypes.data_as(C.c_void_p), _ptr(dev["entries"]), P,
                                                    TRAJ_MODES[align], C.c_int(1 if reflect else 0), _ptr(w_d), _ptr(out),
                                                    _ptr(iout), _ptr(sums), _ptr(scratch), _stream()),
               "nfisam_sample_trajectory_error")
    return dict(theta=out[0], scale=out[1], t=out[2:4], sse_traj=out[4], sse_landmark=out[5], sse_heading=out[6], worst=out[7],
                reflected=iout[0], worst_entry=iout[1], entry_sums=sums[:P], weight_sum=sums[P], n_traj=int((~land).sum()),
                n_landmark=int(land.sum()), n_heading=int((entries["col_th"] >= 0).sum()))


def sample_trajectory_rpe(X, entries: np.ndarray, pairs: np.ndarray, n_slots=None, device=None):
    """Relative pose error of every row of X [n, x_cols] (tensor or numpy) over the pairs of `pairs` (numpy TRAJ_PAIR_DTYPE,
    `pack_traj_pairs`): nfisam_sample_trajectory_rpe, every slot in one launch.  -> dict: trans, rot [n_slots, n] float64 device
    tensors (sum |d_est - d_true|^2 and sum wrap_pi(dth_est - dth_true)^2 over the slot's pairs), count [n_slots] (numpy)."""
    device = _row_major_front("sample_trajectory_rpe", device, X=X)
    if int(X.shape[0]) < 1:
        raise ValueError("sample_trajectory_rpe: no points")
    check_traj_entries(entries, int(X.shape[1]), "none")
    n_slots = check_traj_pairs(pairs, entries, n_slots)
    return sample_trajectory_rpe_t(_columns(X, device), entries, pairs, n_slots, checked=True)


def sample_trajectory_rpe_t(Xt, entries: np.ndarray, pairs: np.ndarray, n_slots=None, checked=False):
    """`sample_trajectory_rpe` on the COLUMN-major matrix Xt [x_rows, n] (a contiguous float32 device tensor, used in place)."""
    x_rows, n = _column_major_front("Xt", Xt)
    device = Xt.device
    if n < 1:
        raise ValueError("sample_trajectory_rpe: no points")
    if not checked:
        check_traj_entries(entries, x_rows, "none")
        n_slots = check_traj_pairs(pairs, entries, n_slots)
    n_slots = int(n_slots)
    entries, pairs = np.ascontiguousarray(entries), np.ascontiguousarray(pairs)
    with torch.cuda.device(device):
        dev = _upload_named(device, entries=_table_bytes(entries), pairs=_table_bytes(pairs))
        out = torch.empty(n_slots, 2, n, dtype=torch.float64, device=device)
        _check(lib().nfisam_sample_trajectory_rpe(_ptr(Xt), x_rows, n, entries.ctypes.data_as(C.c_void_p), _ptr(dev["entries"]),
                                                  int(entries.size), pairs.ctypes.data_as(C.c_void_p), _ptr(dev["pairs"]),
                                                  int(pairs.size), n_slots, _ptr(out), _stream()), "nfisam_sample_trajectory_rpe")
    return dict(trans=out[:, 0], rot=out[:, 1], count=np.bincount(pairs["slot"], minlength=n_slots).astype(np.int64))
