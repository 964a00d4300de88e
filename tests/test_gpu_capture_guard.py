"""The STFT's and the ISTFT's per-call scratch (the per-utterance max words, the frame scratch) never grows while the
call's stream is being captured into a graph: such a call is refused with AVSE_ERR_INVALID and its message says to run
one call of that size first; after that call the same capture succeeds and replays the direct call's bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AVSE_ERR_INVALID = 1
L, T, NB = 3200, 21, 321      # samples, centred frames at hop 160, bins of n_fft 640


def test_stft_istft_scratch_does_not_grow_in_a_capture(gpu):
    from avse_amd import _lib
    lib = _lib.load()
    ctx = _lib.Context(torch.cuda.current_device())   # its own context: scratch sizes no other test has touched
    rng = np.random.default_rng(11)
    sig = torch.from_numpy(rng.normal(0, 3000, (2, L)).astype(np.float32)).cuda()
    mel = torch.zeros((2, 80, T), dtype=torch.float32, device="cuda")
    stft = torch.zeros((2, NB, T, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 160 * (T - 1)), dtype=torch.float32, device="cuda")

    def spec(u, stream):
        return lib.avse_spectrogram(ctx.handle, _lib.ptr(sig), u, L, 16000, 640, 160, 80, 0.0, 8000.0, 1e-5, 80.0,
                                    _lib.AVSE_PAD_REFLECT, 0, _lib.ptr(mel), _lib.ptr(stft), stream)

    def inv(u, stream):
        return lib.avse_istft(ctx.handle, _lib.ptr(mel), _lib.ptr(stft), u, T, T, 0, 16000, 640, 160, 80, 0.0, 8000.0,
                              _lib.ptr(out), stream)

    side = torch.cuda.Stream()
    h = _lib._c_void_p(side.cuda_stream)
    with torch.cuda.stream(side):
        assert spec(1, h) == 0 and inv(1, h) == 0      # tables, and scratch for one utterance
    torch.cuda.synchronize()
    refused = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # two utterances: both calls would have to grow their scratch
        out.zero_()                                    # (a graph of one node: the refused calls add none)
        for name, fn in (("spectrogram", spec), ("istft", inv)):
            refused[name] = (fn(2, h), lib.avse_last_error().decode())
    del graph
    for name, (rc, msg) in refused.items():
        assert rc == AVSE_ERR_INVALID, (name, rc, msg)
        assert f"the {name} scratch would grow while the stream is being captured" in msg, msg
        assert "run one call of this size before the capture" in msg, msg

    with torch.cuda.stream(side):
        assert spec(2, h) == 0 and inv(2, h) == 0      # the call of that size, outside a capture
    torch.cuda.synchronize()
    want = [t.clone() for t in (mel, stft, out)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert spec(2, h) == 0 and inv(2, h) == 0
    for t in (mel, stft, out):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, ref in zip((mel, stft, out), want):
        assert torch.equal(got, ref)
