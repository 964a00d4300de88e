"""CPU tests of the streaming session's host side (avse_stream_*, include/avse.h): the exports, the host-only totals
(avse_stream_counts: frames analysed, slices through the network, samples emitted) and every refusal the C-ABI decides
before it touches a context or the GPU.  The refusals that need a live session are in tests/test_gpu_streaming.py.

The expected totals are the numpy restatement of the semantics, model_counts() below: frame t exists once sample
160 t + 319 has arrived (frame 0: sample 320, its left reflection), a slice needs its 20 frames and its video slice,
and a sample is final once the last frame covering it is inverted."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("avse_stream_create", "avse_stream_counts", "avse_stream_push", "avse_stream_flush", "avse_stream_reset",
           "avse_stream_destroy")


def model_counts(n, v, flushed=False):
    """(frames, slices, emitted) of a stream after n samples and v video slices, from the semantics' own statements."""
    if flushed:
        return 20 * v, v, max(0, 3200 * v - 160)
    frames = 0
    while (n >= 321 if frames == 0 else n >= 160 * frames + 320):
        frames += 1
    slices = min(frames // 20, v)
    return frames, slices, max(0, 3200 * slices - 320)


def test_library_exports_the_streaming_entry_points():
    from avse_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "avse.h")).read()
    assert "typedef struct avse_stream avse_stream;" in header
    for f in SYMBOLS:
        assert hasattr(lib, f) and f in _lib.SIGNATURES, f
        assert re.search(r"\b(int|void)\s+%s\s*\(" % f, header), f"include/avse.h does not declare {f}"
    assert lib.avse_abi_version() == 3          # additive: the ABI version did not move
    assert "avse_stream_push" in header.split("#define AVSE_ABI_VERSION")[0]     # listed in the version comment


def per_push(pushes, v=4):
    from avse_amd import ops
    n, prev, out = 0, 0, []
    for p in pushes:
        n += p
        frames, slices, emitted = ops.stream_counts(n, v)
        assert (frames, slices, emitted) == model_counts(n, v), (pushes, n)
        out.append(emitted - prev)
        prev = emitted
    assert ops.stream_counts(n, v, flushed=True) == model_counts(n, v, True)
    return out, ops.stream_counts(n, v, flushed=True)[2] - prev


@pytest.mark.parametrize("pushes,emitted", [
    ([3200] * 4, [0, 2880, 3200, 3200]),
    ([3360, 3200, 3200, 3040], [2880, 3200, 3200, 0]),
    ([12800], [9280]),
    ([321, 7, 5000, 7472], [0, 0, 2880, 6400]),
])
def test_counts_follow_the_push_pattern(pushes, emitted):
    got, flush = per_push(pushes)
    assert got == emitted and flush == 3360


def test_counts_of_small_pushes():
    got, flush = per_push([1000] * 12 + [800])
    first = next(i for i, e in enumerate(got) if e)
    assert first == 3 and got[first] == 2880 and sum(got) == 9280 and flush == 3360


def test_frame_zero_needs_sample_320():
    from avse_amd import ops
    assert ops.stream_counts(320, 4)[0] == 0 and ops.stream_counts(321, 4)[0] == 1
    assert ops.stream_counts(479, 4)[0] == 1 and ops.stream_counts(480, 4)[0] == 2
    for n in range(0, 7000, 37):
        assert ops.stream_counts(n, 2) == model_counts(n, 2), n


def test_nothing_is_emitted_without_video():
    from avse_amd import ops
    for n in (0, 3200, 12800, 10 ** 6):
        frames, slices, emitted = ops.stream_counts(n, 0)
        assert slices == 0 and emitted == 0 and frames == model_counts(n, 0)[0]
    assert ops.stream_counts(12800, 4)[1:] == (3, 9280)          # the slices complete when the video comes
    assert ops.stream_counts(12800, 2)[1:] == (2, 6080)


def test_counts_refuse_negative_totals_and_an_impossible_flush():
    from avse_amd import _lib
    lib = _lib.load()
    out = [ctypes.c_int64() for _ in range(3)]
    refs = [ctypes.byref(o) for o in out]
    assert lib.avse_stream_counts(None, -1, 0, 0, *refs) == 1
    assert lib.avse_stream_counts(None, 0, -1, 0, *refs) == 1
    assert lib.avse_stream_counts(None, 3201, 1, 1, *refs) == 1 and b"flush" in lib.avse_last_error()
    assert lib.avse_stream_counts(None, 3200, 1, 1, *refs) == 0 and out[2].value == 3040
    assert lib.avse_stream_counts(None, 3200, 1, 0, None, None, None) == 0     # every output is optional


def test_null_and_negative_arguments_are_rejected_without_gpu_work():
    from avse_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n_out = ctypes.c_int64(-7)
    h = ctypes.c_void_p()
    # create: NULL context / weights / out, then bad extents with non-NULL pointers (never read: refused first)
    for ctx, w, out in ((None, p, ctypes.byref(h)), (p, None, ctypes.byref(h)), (p, p, None)):
        rc = lib.avse_stream_create(ctx, w, 2, 16000, 640, 160, 20, 80, 0.0, 8000.0, 1e-5, 80.0, 0, 4, out)
        assert rc == 1 and b"NULL" in lib.avse_last_error()
    for n_streams, max_slices, vdt in ((0, 4, 0), (-1, 4, 0), (2, 0, 0), (2, -3, 0), (2, 4, 7)):
        rc = lib.avse_stream_create(p, p, n_streams, 16000, 640, 160, 20, 80, 0.0, 8000.0, 1e-5, 80.0, vdt, max_slices,
                                    ctypes.byref(h))
        assert rc == 1 and lib.avse_last_error(), (n_streams, max_slices, vdt)
    # geometries that cannot stream are refused before the context is touched too: 29.97 / 30 fps (n_fft 533, hop 133)
    rc = lib.avse_stream_create(p, p, 2, 16000, 533, 133, 24, 80, 0.0, 8000.0, 1e-5, 80.0, 0, 4, ctypes.byref(h))
    assert rc == 3 and b"4 * hop" in lib.avse_last_error()
    rc = lib.avse_stream_create(p, p, 2, 16000, 512, 128, 25, 80, 0.0, 8000.0, 1e-5, 80.0, 0, 4, ctypes.byref(h))
    assert rc == 3          # passes the condition, but no 640-point kernel serves it
    assert not h.value
    # push / flush / reset: a NULL session or count pointer
    assert lib.avse_stream_push(None, p, 16, 16, None, 0, None, None, p, 16, ctypes.byref(n_out), None, None, None) == 1
    assert b"NULL" in lib.avse_last_error()
    assert lib.avse_stream_push(p, p, 16, 16, None, 0, None, None, p, 16, None, None, None, None) == 1
    assert lib.avse_stream_flush(None, None, None, p, 16, ctypes.byref(n_out), None, None, None) == 1
    assert lib.avse_stream_flush(p, None, None, p, 16, None, None, None, None) == 1
    assert lib.avse_stream_reset(None, None) == 1
    # negative counts, missing buffers, a short row stride, half a normaliser: refused before the session is read
    for args in ((p, -1, 16, None, 0, None, None), (p, 16, 16, None, -2, None, None), (None, 16, 16, None, 0, None, None),
                 (p, 16, 16, None, 3, None, None), (p, 16, 8, None, 0, None, None), (p, 16, 16, None, 0, p, None),
                 (p, 16, 16, None, 0, None, p)):
        samples, n_new, stride, video, v_new, vm, vs = args
        rc = lib.avse_stream_push(p, samples, n_new, stride, video, v_new, vm, vs, p, 16, ctypes.byref(n_out), None, None,
                                  None)
        assert rc == 1 and lib.avse_last_error(), args
    assert lib.avse_stream_push(p, p, 16, 16, None, 0, None, None, p, -1, ctypes.byref(n_out), None, None, None) == 1
    assert lib.avse_stream_flush(p, p, None, p, 16, ctypes.byref(n_out), None, None, None) == 1
    assert n_out.value == -7                     # no refused call wrote its count
    lib.avse_stream_destroy(None)                # a NULL session is a no-op


def test_python_bindings_check_their_arguments_on_the_host():
    from avse_amd import _lib, ops
    with pytest.raises(TypeError):
        ops.stream_create(object(), 2)           # weights must be DeviceWeights
    with pytest.raises(_lib.AvseError, match="status 1"):
        ops.stream_counts(-5, 0)
