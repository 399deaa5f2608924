"""The helpers every sample binding stages its arguments with: `_upload_named` (one `upload` for the host arrays present, every
result by name, a tensor brought over as it is), `_entry_f64` (an optional per-entry float64 array in any form) and `_f64` (the
weights, which go the plain way).  On the CPU: `upload` to a non-CUDA device is a plain
copy."""
import numpy as np
import torch

import nfisam_hip as nh


def _counted(monkeypatch):
    calls = []
    real = nh.upload

    def upload(*arrays, **kw):
        calls.append(len(arrays))
        return real(*arrays, **kw)

    monkeypatch.setattr(nh, "upload", upload)
    return calls


def test_upload_named_makes_one_upload_and_maps_absent_names_to_none(monkeypatch):
    calls = _counted(monkeypatch)
    blocks = nh.pack_mmd_blocks([2, 3], [1.0, 0.5])
    given = dict(blocks=blocks.view(np.uint8).reshape(-1), cols=np.array([4, 0, 2, 1, 3], dtype=np.int32), scale=None,
                 wrap=np.array([0, 0, 1, 0, 1], dtype=np.uint8), center=np.array([[0.5, -1.25], [3.0, 1e-300]]), weights=None)
    dev = nh._upload_named("cpu", **given)
    assert calls == [4]                                                # one call, the four arrays present
    assert list(dev) == list(given)                                    # every name, in the order given
    for name, a in given.items():
        if a is None:
            assert dev[name] is None
        else:
            t = dev[name]
            assert torch.is_tensor(t) and t.dtype == nh._TORCH_OF[a.dtype.type] and tuple(t.shape) == a.shape, name
            assert np.array_equal(t.numpy(), a), name
    # an absent array in front of a present one does not shift the others
    dev = nh._upload_named("cpu", scale=None, wrap=given["wrap"])
    assert calls == [4, 1] and dev["scale"] is None and np.array_equal(dev["wrap"].numpy(), given["wrap"])


def test_upload_named_with_nothing_present_uploads_nothing(monkeypatch):
    calls = _counted(monkeypatch)
    assert nh._upload_named("cpu", scale=None, wrap=None) == dict(scale=None, wrap=None)
    assert nh._upload_named("cpu") == {}
    assert calls == []


def test_f64_takes_none_numpy_and_tensors():
    assert nh._f64(None, "cpu") is None
    for a in (np.array([1, 2, 3]), np.array([0.1, 0.2, 0.3], dtype=np.float32), [0.5, 1.5]):
        t = nh._f64(a, "cpu")
        assert t.dtype == torch.float64 and t.is_contiguous() and t.device.type == "cpu"
        assert np.array_equal(t.numpy(), np.asarray(a).astype(np.float64))
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()[1]     # a strided float32 CPU tensor
    assert not src.is_contiguous()
    t = nh._f64(src, "cpu")
    assert t.dtype == torch.float64 and t.is_contiguous() and torch.equal(t, src.double())


def test_a_per_entry_array_reaches_its_name_in_every_form(monkeypatch):
    """None, a list, numpy of another dtype and a CPU tensor: the name maps to None or to the float64 values, and what `wrap`
    maps to does not depend on the form `scale` came in.  (A device tensor stays a tensor and is not staged: the GPU test.)"""
    calls = _counted(monkeypatch)
    wrap = np.array([1, 0, 1], dtype=np.uint8)
    want = np.array([0.5, 2.0, 3.0])
    assert nh._entry_f64(None) is None
    for scale in ([0.5, 2, 3], want.astype(np.float32), torch.tensor([0.5, 2.0, 3.0]), torch.from_numpy(want)):
        staged = nh._entry_f64(scale)
        assert isinstance(staged, np.ndarray) and staged.dtype == np.float64 and staged.flags.c_contiguous
        dev = nh._upload_named("cpu", scale=staged, wrap=wrap)
        assert dev["scale"].dtype == torch.float64 and np.array_equal(dev["scale"].numpy(), want)
        assert np.array_equal(dev["wrap"].numpy(), wrap)
    assert calls == [2, 2, 2, 2]
    # a value that is a tensor already is brought over by name and is not part of the upload
    del calls[:]
    strided = torch.arange(6, dtype=torch.float64)[::2]
    dev = nh._upload_named("cpu", scale=strided, wrap=wrap, center=None)
    assert calls == [1] and dev["center"] is None and np.array_equal(dev["wrap"].numpy(), wrap)
    assert dev["scale"].is_contiguous() and torch.equal(dev["scale"], strided)
    dev = nh._upload_named("cpu", scale=strided, wrap=None)          # nothing on the host: no upload at all
    assert calls == [1] and dev["wrap"] is None and torch.equal(dev["scale"], strided)
