"""The optional arguments of the sample bindings in all the forms they are accepted in (None, list, numpy, device tensor):
every form gives the bits of the explicit neutral value or of the same values in another form, and every binding call stages
its small host arrays with exactly ONE `upload`.

No tolerance is involved.  The kernels read an absent array as its neutral value (scale 1, wrap / circular 0, weight 1, center
0) and then run the same float64 operations in the same order, and x * 1.0, x - 0.0 and x + 0.0 are exact; the form an array
arrives in changes how it reaches the device, never its values.

Shapes: 70 points (modes: two groups of 64 starts, the second partial; quantiles: padded to 128 keys), MMD 70 x 65 (two tiles
a side, the second partial), two blocks of widths 2 and 3, the last column of the second an angle."""
import numpy as np
import pytest
import torch

import nfisam_hip as nh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLS = np.arange(5, dtype=np.int32)
WRAP = np.array([0, 0, 0, 0, 1], dtype=np.uint8)
SCALE = np.array([0.5, 2.0, 1.5, 0.25, 3.0])
PROBS = [0.0, 0.1, 0.5, 0.9, 1.0]
MODES_KW = dict(tol=0.0, max_iters=5)


def _points(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 5))
    x[:, :2] += np.where(rng.random(n) < 0.5, -2.0, 2.0)[:, None]
    x[:, 4] = rng.uniform(-np.pi, np.pi, size=n)
    return x.astype(np.float32)


def _same(a, b):
    """Equal element by element, with no tolerance, NaN equal to NaN (torch's equality: -0.0 == 0.0), on tensors, tuples of
    tensors and dicts of tensors."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        return bool(torch.allclose(a, b, rtol=0.0, atol=0.0, equal_nan=True))
    return bool(torch.equal(a, b))


def test_optional_arguments_in_every_form(monkeypatch):
    uploads = []
    real_upload = nh.upload

    def counted(*arrays, **kw):
        uploads.append(len(arrays))
        return real_upload(*arrays, **kw)

    monkeypatch.setattr(nh, "upload", counted)

    def call(fn, *args, **kw):
        del uploads[:]
        out = fn(*args, **kw)
        assert len(uploads) == 1, (fn.__name__, uploads)
        return out

    X, Y = _points(70, 7), _points(65, 8)
    Xt = torch.from_numpy(X).to(DEV).t().contiguous()
    Yt = torch.from_numpy(Y).to(DEV).t().contiguous()
    rng = np.random.default_rng(9)
    w = rng.uniform(0.5, 1.5, size=70)
    w_d = torch.from_numpy(w).to(DEV)
    center = rng.uniform(-1.0, 1.0, size=5)
    center_d = torch.from_numpy(center).to(DEV)
    scale_d = torch.from_numpy(SCALE).to(DEV)
    ones, zeros = np.ones(5), np.zeros(5, dtype=np.uint8)

    # ---- MMD: scale (None, list, numpy) x wrap (None, given) -------------------------------------------------------------------
    blocks = nh.pack_mmd_blocks([2, 3], [1.0, 1.3])
    base = call(nh.mmd_sums, X, Y, blocks, COLS, COLS, device=DEV)
    assert base.shape == (2, 3) and bool(torch.isfinite(base).all())
    assert torch.equal(base, call(nh.mmd_sums, X, Y, blocks, COLS, COLS, scale=ones, wrap=zeros, device=DEV))
    assert torch.equal(base, call(nh.mmd_sums, X, Y, blocks, COLS, COLS, scale=list(ones), device=DEV))
    assert torch.equal(base, call(nh.mmd_sums_t, Xt, Yt, blocks, COLS, COLS, wrap=zeros))
    for wrap in (None, WRAP):
        ref = call(nh.mmd_sums, X, Y, blocks, COLS, COLS, scale=ones, wrap=wrap, device=DEV)
        assert torch.equal(ref, call(nh.mmd_sums_t, Xt, Yt, blocks, COLS, COLS, wrap=wrap))
        got = call(nh.mmd_sums, X, Y, blocks, COLS, COLS, scale=list(SCALE), wrap=wrap, device=DEV)
        assert torch.equal(got, call(nh.mmd_sums_t, Xt, Yt, blocks, COLS, COLS, scale=SCALE, wrap=wrap))
        assert not torch.equal(got, ref)                           # (the scale reached the kernel)
        # ... and as a CPU tensor, float64 and float32 (these values are exact in both)
        for sc in (torch.from_numpy(SCALE), torch.tensor(SCALE, dtype=torch.float32)):
            assert torch.equal(got, call(nh.mmd_sums_t, Xt, Yt, blocks, COLS, COLS, scale=sc, wrap=wrap, checked=True))

    # ---- moments: weights (None, numpy, device) x circular (None, given) -------------------------------------------------------
    mblocks = nh.pack_moment_blocks([2, 3])
    base = call(nh.sample_moments, X, mblocks, COLS, device=DEV)
    assert _same(base, call(nh.sample_moments, X, mblocks, COLS, circular=zeros, weights=np.ones(70), device=DEV))
    assert _same(base, call(nh.sample_moments_t, Xt, mblocks, COLS, weights=torch.ones(70, dtype=torch.float64, device=DEV)))
    for circ in (None, WRAP):
        ref = call(nh.sample_moments, X, mblocks, COLS, circular=circ, weights=np.ones(70), device=DEV)
        assert _same(ref, call(nh.sample_moments_t, Xt, mblocks, COLS, circular=circ))
        assert bool(torch.isnan(ref[1][:4]).all())                 # a Euclidean entry has no resultant length
        got = call(nh.sample_moments, X, mblocks, COLS, circular=circ, weights=w, device=DEV)
        assert _same(got, call(nh.sample_moments_t, Xt, mblocks, COLS, circular=circ, weights=w_d))
        assert _same(got, call(nh.sample_moments, X, mblocks, COLS, circular=circ, weights=w_d, device=DEV))
        assert not _same(got, ref)

    # ---- quantiles: center (None, numpy, device) x circular (None, given) ------------------------------------------------------
    base = call(nh.sample_quantiles, X, COLS, PROBS, device=DEV)
    assert base.shape == (5, 5)
    assert torch.equal(base, call(nh.sample_quantiles, X, COLS, PROBS, circular=zeros, center=np.zeros(5), device=DEV))
    assert torch.equal(base, call(nh.sample_quantiles_t, Xt, COLS, PROBS, center=center_d))    # no angle: the center is not read
    assert torch.equal(base, call(nh.sample_quantiles_t, Xt, COLS, PROBS, center=center))
    ref = call(nh.sample_quantiles, X, COLS, PROBS, circular=WRAP, device=DEV)
    assert torch.equal(ref, call(nh.sample_quantiles_t, Xt, COLS, PROBS, circular=WRAP, center=np.zeros(5)))
    assert torch.equal(ref, call(nh.sample_quantiles_t, Xt, COLS, PROBS, circular=WRAP,
                                 center=torch.zeros(5, dtype=torch.float64, device=DEV)))
    got = call(nh.sample_quantiles, X, COLS, PROBS, circular=WRAP, center=center, device=DEV)
    assert torch.equal(got, call(nh.sample_quantiles_t, Xt, COLS, PROBS, circular=WRAP, center=center_d))
    assert torch.equal(got, call(nh.sample_quantiles, X, COLS, PROBS, circular=list(WRAP), center=center_d, device=DEV))
    assert torch.equal(got[:4], ref[:4]) and not torch.equal(got[4], ref[4])

    # ---- modes: scale (None, list, numpy, device) x wrap (None, given) x weights (None, numpy, device) -------------------------
    base = call(nh.sample_modes, X, blocks, COLS, device=DEV, **MODES_KW)
    assert base["pos"].shape == (5, 70) and base["labels"].shape == (2, 70)
    assert _same(base, call(nh.sample_modes, X, blocks, COLS, scale=ones, wrap=zeros, weights=np.ones(70), device=DEV, **MODES_KW))
    assert _same(base, call(nh.sample_modes_t, Xt, blocks, COLS, scale=torch.ones(5, dtype=torch.float64, device=DEV), **MODES_KW))
    for wrap in (None, WRAP):
        # the neutral scale in its three forms: absent, on the host, on the device
        ref = call(nh.sample_modes, X, blocks, COLS, wrap=wrap, device=DEV, **MODES_KW)
        assert _same(ref, call(nh.sample_modes_t, Xt, blocks, COLS, scale=list(ones), wrap=wrap, **MODES_KW))
        assert _same(ref, call(nh.sample_modes_t, Xt, blocks, COLS, scale=torch.ones(5, dtype=torch.float64, device=DEV), wrap=wrap,
                               **MODES_KW))
        for weights, weights_dev in ((None, None), (w, w_d)):
            got = call(nh.sample_modes, X, blocks, COLS, scale=list(SCALE), wrap=wrap, weights=weights, device=DEV, **MODES_KW)
            assert _same(got, call(nh.sample_modes_t, Xt, blocks, COLS, scale=SCALE, wrap=wrap, weights=weights_dev, **MODES_KW))
            assert _same(got, call(nh.sample_modes_t, Xt, blocks, COLS, scale=scale_d, wrap=wrap, weights=weights, **MODES_KW))
            assert not _same(got["pos"], ref["pos"])
            # the merge alone, on that call's points, in the host and the device form of the scale
            for sc in (SCALE, scale_d):
                again = call(nh.sample_modes_merge_t, got, 5, blocks, COLS, scale=sc, wrap=wrap, weights=weights_dev)
                assert again["pos"] is got["pos"] and again["dens"] is got["dens"]
                for k in ("labels", "n_modes", "mode_pos", "mode_dens", "mode_mass", "unlabelled"):
                    assert _same(again[k], got[k]), k
    assert int(base["n_modes"].min()) >= 1
