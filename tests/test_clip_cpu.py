"""Per-parameter gradient clipping on the device (csrc/tan_clip.hip), the host side: the chunk / segment tables `_Flat.clip_tables()`
hands the kernels, and the fp64 restatement of the reference rule (utils/train_utils.py:3-13) that tests/test_clip_gpu.py measures the
kernels against.  No GPU."""
import numpy as np
import torch

from temporalalignnet_amd import ops
from temporalalignnet_amd.tan_model import TemporalAligner, TwinTemporalAligner


def clip_rule_fp64(g, clip, grad_scale=1.0):
    """clip_gradients() for ONE tensor in fp64: (norm, clipped gradient, whether it was clipped).  `grad_scale` is what the
    optimizer multiplies the stored gradient by afterwards (1 / world size): the norm is that of the scaled gradient, the stored
    gradient stays unscaled (train.py `optimizer_step`)."""
    g = np.asarray(g, dtype=np.float64)
    norm = np.sqrt(np.sum(g * g)) * grad_scale              # param_norm = p.grad.data.norm(2)
    coef = clip / (norm + 1e-6)                             # clip_coef = clip_grad / (param_norm + 1e-6)
    clipped = bool(coef < 1)                                # if clip_coef < 1: p.grad.data.mul_(clip_coef)
    return norm, (g * coef if clipped else g), clipped


def test_fp64_restatement_follows_the_reference_rule():
    # above the threshold: ||(3, 4)|| = 5 > 1 -> scaled by 1 / (5 + 1e-6)
    norm, out, clipped = clip_rule_fp64([3.0, 4.0], 1.0)
    assert clipped and norm == 5.0
    np.testing.assert_allclose(out, [3.0 / 5.000001, 4.0 / 5.000001], rtol=1e-15)
    np.testing.assert_allclose(np.sqrt(np.sum(out * out)), 1.0 - 2e-7, rtol=1e-9)          # the norm lands just under the threshold
    # below: ||(0.3, 0.4)|| = 0.5 -> coef = 2 / (1 + 2e-6) >= 1: untouched, bit for bit
    norm, out, clipped = clip_rule_fp64([0.3, 0.4], 1.0)
    assert not clipped and abs(norm - 0.5) < 1e-15 and np.array_equal(out, np.asarray([0.3, 0.4]))
    # all zero: coef = clip / 1e-6 -- no division by zero, untouched
    norm, out, clipped = clip_rule_fp64(np.zeros(5), 1.0)
    assert not clipped and norm == 0.0 and np.array_equal(out, np.zeros(5))
    # the optimizer's scale moves the norm, not the stored gradient: (3, 4) / 8 has norm 0.625 < 1
    norm, out, clipped = clip_rule_fp64([3.0, 4.0], 1.0, grad_scale=0.125)
    assert not clipped and norm == 0.625 and np.array_equal(out, np.asarray([3.0, 4.0]))
    norm, out, clipped = clip_rule_fp64([3.0, 4.0], 0.5, grad_scale=0.125)
    assert clipped and norm == 0.625
    np.testing.assert_allclose(out, np.asarray([3.0, 4.0]) * 0.5 / 0.625001, rtol=1e-15)
    # and the rule as the reference spells it, on torch tensors in fp64
    rng = np.random.default_rng(0)
    for scale in (10.0, 0.01):
        g = rng.standard_normal(37) * scale
        t = torch.from_numpy(g.copy())
        param_norm = t.norm(2)
        clip_coef = 3.0 / (param_norm + 1e-6)
        if clip_coef < 1:
            t.mul_(clip_coef)
        norm, out, clipped = clip_rule_fp64(g, 3.0)
        assert clipped == (scale == 10.0)
        np.testing.assert_allclose(norm, param_norm.item(), rtol=1e-14)
        np.testing.assert_allclose(out, t.numpy(), rtol=1e-14)


def _check_tables(f):
    t = f.clip_tables()
    chunk = ops.clip_chunk()
    assert t.chunk == chunk and chunk >= 1024 and chunk & (chunk - 1) == 0
    assert t.chunks.dtype == np.int32 and t.chunks.shape[1] == 4 and t.segs.dtype == np.int32 and t.segs.shape == (len(t.names), 2)
    assert f.total < 2 ** 31
    # every parameter exactly once
    assert sorted(t.names) == sorted(f.names) and len(set(t.names)) == len(t.names)
    # chunks tile each segment exactly, in order, and a segment's chunks are consecutive
    owner = np.full(f.total, -1, dtype=np.int64)
    nxt = 0
    for s, n in enumerate(t.names):
        o, k, _ = f.off[n]
        first, cnt = (int(v) for v in t.segs[s])
        assert first == nxt and cnt == (k + chunk - 1) // chunk
        pos = o
        for c in range(first, first + cnt):
            off, ln, seg, zero = (int(v) for v in t.chunks[c])
            assert off == pos and seg == s and zero == 0 and 0 < ln <= chunk
            assert ln == chunk or c == first + cnt - 1                       # (only a segment's last chunk is short)
            assert (owner[off:off + ln] == -1).all()
            owner[off:off + ln] = s
            pos += ln
        assert pos == o + k
        nxt = first + cnt
    assert nxt == t.chunks.shape[0]
    # ... and never a padding element: what no parameter owns, no chunk owns
    param = np.zeros(f.total, dtype=bool)
    for n in f.names:
        o, k, _ = f.off[n]
        param[o:o + k] = True
    assert np.array_equal(owner >= 0, param)
    # the three groups: contiguous ranges of chunks and segments, in the order the optimizer steps them
    cb, sb = t.chunk_bounds, t.seg_bounds
    assert len(cb) == len(sb) == 4 and cb[0] == sb[0] == 0 and cb[3] == t.chunks.shape[0] and sb[3] == len(t.names)
    assert list(cb) == sorted(cb) and list(sb) == sorted(sb)
    for g in range(3):
        assert sb[g] < sb[g + 1] and cb[g] < cb[g + 1]
        assert cb[g] == int(t.segs[sb[g], 0]) and cb[g + 1] == int(t.segs[sb[g + 1] - 1].sum())
    is_mat = lambda n: ".resblocks." in n and len(f.off[n][2]) == 2              # noqa: E731
    for s, n in enumerate(t.names):
        g = 0 if s < sb[1] else (1 if s < sb[2] else 2)
        want = 2 if not is_mat(n) else (0 if n.startswith("video_temporal_encoder.") else 1)
        assert g == want, (n, g, want)
        if g == 1:
            assert n.startswith("joint_temporal_encoder.")
    return t


def test_clip_tables_cover_every_parameter_in_three_groups():
    m = TemporalAligner(2, 3, language_model=None)
    t = _check_tables(m._flat)
    # the matrices of a block: in_proj, out_proj, c_fc, c_proj
    assert t.seg_bounds[1] == 2 * 4 and t.seg_bounds[2] - t.seg_bounds[1] == 3 * 4
    assert m._flat.clip_tables() is t                                        # built once
    # the largest matrix (c_fc / c_proj: 2048 x 512) takes 2048 * 512 / chunk chunks
    assert int(t.segs[:, 1].max()) == 2048 * 512 // t.chunk
    # the group boundaries are the optimizer's unit boundaries: units of 64 x 64 elements over the same matrices, in the same order
    elems = [sum(int(t.chunks[c, 1]) for c in range(t.chunk_bounds[g], t.chunk_bounds[g + 1])) for g in range(2)]
    assert elems[0] == 2 * (3 + 1 + 4 + 4) * 512 * 512 and elems[1] == 3 * (3 + 1 + 4 + 4) * 512 * 512


def test_each_flat_buffer_of_a_twin_has_its_own_tables():
    tw = TwinTemporalAligner(0.999, num_encoder_layers=1, num_decoder_layers=3, use_alignability_head=1, language_model=None)
    a, b = _check_tables(tw.online._flat), _check_tables(tw.target._flat)
    assert a is not b and a.chunks is not b.chunks
    f = tw.online._flat
    assert f.total > sum(f.off[n][1] for n in f.names)                       # (the head's bias is one element: this model has padding)
    assert a.names == b.names and np.array_equal(a.chunks, b.chunks) and np.array_equal(a.segs, b.segs)
    assert any("binary_head" in n for n in a.names[a.seg_bounds[2]:])        # the alignability head: with "everything else"
