"""pipeline.Enhancer with slices that have no video (video_present): every slice is predicted as the clip it would have
been alone (tests/test_gpu_forward_mixed.py), so the enhanced signal is the ISTFT of those per-slice predictions, bit
for bit, in the batched and in the ragged form."""
import functools

import numpy as np
import pytest
import torch

from conftest import synth_audio, synth_video
from oracle import librosa_ref as R

pytestmark = pytest.mark.gpu

U, S, SLICE = 2, 3, 3200
MASK = np.array([[1, 0, 1], [0, 1, 1]], bool)     # one slice without video per utterance


@functools.lru_cache(None)
def setup():
    from avse_amd import ops
    from avse_amd.model import KerasModel
    rng = np.random.default_rng(77)
    x = synth_audio(rng, U, S * SLICE)
    video = synth_video(rng, U * S).reshape(U, S, 128, 128, 5)
    mean, std = R.video_normalizer_fit(video.reshape(U * S, 128, 128, 5))
    dw = ops.DeviceWeights(KerasModel.init(seed=9, randomize=True), "float32_split")
    return x, video, ops.to_device(mean), ops.to_device(std), dw


def reference(x, video, mask, md, sd, dw):
    """ISTFT of the per-slice predictions: forward(video)[i] where the slice has video, forward(video=None)[i] where
    it has not, on the mel slices and the mixture phase of the plain pipeline."""
    from avse_amd import ops
    u, s = mask.shape
    mel, stft = ops.spectrogram(ops.to_device(x), frames_per_slice=20, return_stft=True)
    clips = mel.view(u * s, 80, 20)
    full = ops.forward(dw, clips, ops.to_device(video.reshape(u * s, 128, 128, 5)), md, sd)
    none = ops.forward(dw, clips, None)
    keep = torch.from_numpy(mask.reshape(-1)).to(full.device)[:, None, None]
    pred = torch.where(keep, full, none)
    assert not torch.equal(full, none)
    return ops.istft(pred.view(u, s, 80, 20), stft).cpu().numpy()


def garbage_where_blank(video, mask):
    """The caller's video keeps its shape; what the slices without video hold is never read"""
    v = video.copy()
    v[~mask] = np.float32(3e38)
    return v


def test_enhancer_call_with_blank_slices(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    x, video, md, sd, dw = setup()
    ref = reference(x, video, MASK, md, sd, dw)
    enh = Enhancer(dw)
    got = enh(ops.to_device(x), ops.to_device(garbage_where_blank(video, MASK)), md, sd, video_present=MASK)
    assert enh.range_bits == 0
    assert np.array_equal(got.cpu().numpy(), ref)
    # chunks that are all present, all blank and mixed (chunk = 2 over the 6 clips: [1, 0] [1, 0] [1, 1])
    got2 = Enhancer(dw, chunk=2)(ops.to_device(x), ops.to_device(garbage_where_blank(video, MASK)), md, sd,
                                 video_present=torch.from_numpy(MASK))
    assert np.array_equal(got2.cpu().numpy(), ref)
    with pytest.raises(ValueError, match="video_present"):
        enh(ops.to_device(x), ops.to_device(video), md, sd, video_present=MASK[:, :2])


def test_enhance_ragged_with_blank_slices(gpu):
    from avse_amd import ops
    from avse_amd.pipeline import Enhancer
    x, video, md, sd, dw = setup()
    lens = [2, 3]
    masks = [MASK[0, :2], MASK[1]]
    sigs = [ops.to_device(x[u, :n * SLICE]) for u, n in enumerate(lens)]
    vids = [ops.to_device(garbage_where_blank(video[u, :n], masks[u])) for u, n in enumerate(lens)]
    got = Enhancer(dw).enhance_ragged(sigs, vids, md, sd, video_present=masks)
    for u, n in enumerate(lens):
        ref = reference(x[u:u + 1, :n * SLICE], video[u:u + 1, :n], masks[u][None], md, sd, dw)
        assert np.array_equal(got[u].cpu().numpy(), ref[0]), u
