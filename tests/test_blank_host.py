"""CPU tests of the forward for batches with clips that have no video (include/avse.h avse_forward_mixed): the additive
entry points and what the library and ops.forward refuse on the host, before any GPU work."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest

MIXED_ENTRY_POINTS = ("avse_forward_mixed", "avse_forward_mixed_checked", "avse_stream_push_each_mixed",
                      "avse_stream_blank")


def test_library_exports_the_mixed_entry_points():
    from avse_amd import _lib
    lib = _lib.load()
    header = open(_lib.HEADER_PATH).read()
    version_comment = header[header.index("/* 2: compute dtype"):header.index("#define AVSE_ABI_VERSION")]
    for f in MIXED_ENTRY_POINTS:
        assert hasattr(lib, f) and f in _lib.SIGNATURES, f
        assert re.search(rf"\b{f}\b", version_comment), f     # listed with the other additions under version 3
        assert re.search(rf"^int {f}\(", header, re.M), f
    assert lib.avse_abi_version() == 3 and "#define AVSE_ABI_VERSION 3" in header


def test_library_refuses_bad_masks_before_the_context_is_touched():
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))      # non-NULL dummy, never read
    one = (ctypes.c_uint8 * 2)(0, 1)
    bits = ctypes.c_uint32(9)
    # present == NULL; video == NULL with a clip marked; N out of range (the mask is not read)
    assert lib.avse_forward_mixed(p, p, p, p, 0, None, None, None, 2, p, None) == 1
    assert b"present" in lib.avse_last_error()
    assert lib.avse_forward_mixed(p, p, p, None, 0, None, None, one, 2, p, None) == 1
    assert b"video == NULL" in lib.avse_last_error()
    assert lib.avse_forward_mixed(p, p, p, p, 0, None, None, one, -1, p, None) == 1
    assert lib.avse_forward_mixed(p, p, p, p, 0, p, None, one, 2, p, None) == 1
    assert b"vnorm" in lib.avse_last_error()
    assert lib.avse_forward_mixed_checked(p, p, p, None, 0, None, None, one, 2, p, None, 0, ctypes.byref(bits)) == 1
    assert bits.value == 0


def test_ops_forward_refuses_bad_masks_before_touching_the_library(monkeypatch):
    import torch
    from avse_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "context", no_library)
    weights = SimpleNamespace(T=20, F=5)
    audio = torch.zeros(4, 80, 20)
    video = torch.zeros(2, 128, 128, 5)
    for mask in ([True, False, True], np.ones(5, bool), np.ones((4, 1), bool), []):
        with pytest.raises(ValueError, match="video_present"):
            ops.forward(weights, audio, video, video_present=mask)
    for mask in ([True, False, False, False], [True] * 4, np.array([1, 1, 0, 1], bool)):
        with pytest.raises(ValueError, match="packed"):
            ops.forward(weights, audio, video, video_present=mask)
    with pytest.raises(ValueError, match="packed"):
        ops.forward(weights, audio, None, video_present=[False, True, False, False])
    with pytest.raises(ValueError, match="packed"):
        ops.forward(weights, audio, video, video_present=[False] * 4)
    m = ops.present_mask(torch.tensor([True, False, True, False]), 4, 2)
    assert m.dtype == np.uint8 and m.flags.c_contiguous and m.tolist() == [1, 0, 1, 0]


def test_no_video_entries_are_refused_on_the_host(monkeypatch):
    from avse_amd import _lib, ops, pipeline

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="NoVideo"):
            pipeline.NoVideo(bad)
    assert pipeline.NoVideo is ops.NoVideo and pipeline.NoVideo(3).k == 3
    enh = object.__new__(pipeline.StreamEnhancer)      # a retimed enhancer, as far as push_each looks before the library
    enh.retimer, enh.input_rate = object(), None
    for video in ([pipeline.NoVideo(1), None], [None, [pipeline.NoVideo(2)]]):
        with pytest.raises(ValueError, match="input_fps"):
            enh.push_each(video=video)
    enh.session = SimpleNamespace(n_streams=2)
    with pytest.raises(ValueError, match="input_fps"):
        enh.push(None, pipeline.NoVideo(1))
