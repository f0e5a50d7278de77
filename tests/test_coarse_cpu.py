"""Coarse-to-fine search without a GPU: the reference of the MXFP4 row format against the header's worked examples, the continued
top list and the per-shard cutoff rule, the candidate union and back-mapping of `search/coarse.py` over a stand-in for `ops`, and
the argument checks of `search(..., coarse=)`, the C entry points and the command line."""
import ctypes as C

import numpy as np
import pytest
import torch

import coarse_ref as ref
from temporalalignnet_amd import _lib
from temporalalignnet_amd import search as srch
from temporalalignnet_amd.search import coarse as c2f


# ------------------------------------------------------------------------------------------------------------- the reference quantiser
def _block(values, fill=0.0):
    row = np.full(512, fill, dtype=np.float32)
    row[:len(values)] = values
    return row[None]


def _nibbles(codes):
    return np.stack((codes & 15, codes >> 4), -1).reshape(codes.shape[0], 512)


def test_every_tie_goes_to_the_even_code():
    # amax 6: s = 0 (6 = 0.75 * 2^3), the block is on the grid itself
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    codes, scales = ref.quantize(_block([6.0] + ties + [-t for t in ties]))
    assert scales[0, 0] == 127 and (scales[0, 1:] == 127).all()
    nib = _nibbles(codes)[0]
    assert nib[0] == 7
    assert nib[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]                            # 0, 1, 1, 2, 2, 4, 4
    assert nib[8:15].tolist() == [8, 10, 10, 12, 12, 14, 14]                      # the sign bit is x's, also where the magnitude is 0
    assert ref.dequantize(codes, scales)[0, :8].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    up = [np.nextafter(np.float32(t), np.float32(9)) for t in ties]
    down = [np.nextafter(np.float32(t), np.float32(0)) for t in ties]
    nib = _nibbles(ref.quantize(_block([6.0] + up + down))[0])[0]
    assert nib[1:8].tolist() == [1, 2, 3, 4, 5, 6, 7] and nib[8:15].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert _nibbles(ref.quantize(_block([6.0, -0.0, -0.1, 0.1]))[0])[0, 1:4].tolist() == [8, 8, 0]


def test_the_block_scale_at_the_edge_and_at_zero():
    for e in (-100, -3, 0, 1, 60):
        at = np.ldexp(np.float32(0.75), e)
        above = np.nextafter(at, np.float32(np.inf))
        half = np.ldexp(np.float32(0.5), e)
        assert ref.quantize(_block([at]))[1][0, 0] == e - 3 + 127                 # amax * 2^-s == 6
        assert ref.quantize(_block([above]))[1][0, 0] == e - 2 + 127              # just above 3
        assert ref.quantize(_block([half]))[1][0, 0] == e - 3 + 127               # == 4
        assert _nibbles(ref.quantize(_block([at]))[0])[0, 0] == 7 and _nibbles(ref.quantize(_block([-half]))[0])[0, 0] == 14
    codes, scales = ref.quantize(np.zeros((1, 512), dtype=np.float32))            # a zero row
    assert (scales == 127).all() and (codes == 0).all()
    x = np.ones((1, 512), dtype=np.float32)
    x[0, 64:96] = 0                                                               # a zero block
    codes, scales = ref.quantize(x)
    assert scales[0, 2] == 127 and (codes[0, 32:48] == 0).all() and scales[0, 0] == 127 - 2      # 1 = 0.5 * 2^1: s = -2, code 4.0
    assert (_nibbles(codes)[0, :64] == 6).all()


def test_blocks_across_the_binades_never_saturate_and_the_scale_clamps():
    rng = np.random.default_rng(0)
    e = rng.integers(-149, 127, (400, 16, 1))
    x = np.ldexp(rng.uniform(-1, 1, (400, 16, 32)), e).astype(np.float32).reshape(400, 512)
    y, s = ref.scaled_blocks(x)
    amax = np.abs(y).max(-1)
    live = np.abs(x.reshape(400, 16, 32)).max(-1) > 0
    assert (amax <= 6).all() and s.min() == -127 and s.max() <= 127
    unclamped = live & (s > -127)
    assert (amax[unclamped] > 3).all()
    codes, scales = ref.quantize(x)
    assert scales.max() < 255 and scales.min() == 0
    err = np.abs(ref.dequantize(codes, scales) - x.astype(np.float64)).reshape(400, 16, 32)
    assert (err <= np.ldexp(1.0, s)[..., None]).all()                             # half of e2m1's widest gap (2), scaled


def test_e4m3_values_are_the_hosts():
    c = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(c).view(torch.float8_e4m3fn).double().numpy()
    got = ref.e4m3_values(c)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ------------------------------------------------------------------------------------------------------------------ continued lists
def test_a_continued_list_equals_the_one_shot_list():
    rng = np.random.default_rng(1)
    scores = rng.integers(0, 12, (9, 200)).astype(np.float32)                     # many equal scores
    s32, r32 = ref.top_lists(scores, 32)
    s16, r16 = ref.top_lists(scores, 16)
    s2, r2 = ref.top_lists(scores, 16, (s16[:, -1], r16[:, -1]))
    assert np.array_equal(np.concatenate((r16, r2), 1), r32) and np.array_equal(np.concatenate((s16, s2), 1), s32)
    assert (s32[:, 15] == s32[:, 16]).any()
    none = ref.top_lists(scores, 4, (np.full(9, -1.0, dtype=np.float32), np.full(9, ref.EMPTY_ROW)))
    assert (none[1] == ref.EMPTY_ROW).all() and np.isinf(none[0]).all()
    assert np.array_equal(ref.top_lists(scores, 5, (np.full(9, 11.0, dtype=np.float32), np.full(9, -1)))[1], r32[:, :5])


def test_three_rounds_over_three_shards_with_ties_across_the_shard_boundaries():
    rng = np.random.default_rng(2)
    shards = [rng.integers(0, 4, (6, n)).astype(np.float32) for n in (17, 40, 23)]          # four score values: ties everywhere
    whole = np.concatenate(shards, 1)
    base = np.cumsum([0, 17, 40])
    one_s, one_r = ref.top_lists(whole, 30)
    for q in range(6):
        got, below = [], None
        for _ in range(3):
            lists = []
            for s, sc in enumerate(shards):
                cut = None if below is None else (below[0], int(ref.shard_cutoff_row(below[1], below[2], s)))
                lists.append(ref.top_list(sc[q], 10, cut))
            f = ref.fold(lists, 10)
            got.append(f)
            below = (f[0][-1], f[1][-1], f[2][-1])
        score = np.concatenate([g[0] for g in got])
        row = np.concatenate([base[g[1]] + g[2] for g in got])
        assert np.array_equal(row, one_r[q]) and np.array_equal(score, one_s[q])
    assert ref.shard_cutoff_row(np.array([1, 1, 1]), np.array([5, 5, 5]), 0).tolist() == [ref.EMPTY_ROW] * 3
    assert ref.shard_cutoff_row(np.array([1]), np.array([5]), 1).tolist() == [5]
    assert ref.shard_cutoff_row(np.array([1]), np.array([5]), 2).tolist() == [-1]
    dev = c2f.shard_cutoff_row(torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([5, 6, 7], dtype=torch.int32), 1)
    assert dev.tolist() == ref.shard_cutoff_row(np.array([0, 1, 2]), np.array([5, 6, 7]), 1).tolist() == [-1, 6, ref.EMPTY_ROW]


# ------------------------------------------------------------------------------------------- candidate union and back-mapping
class _DenseOps:
    """`ops` as `search/coarse.py` uses it, over CPU tensors: the coarse sweep ranks a dense noisy score matrix, the exact sweep the
    dense product of the rows it is handed, the fold is coarse_ref's."""

    def __init__(self, coarse_scores):
        self.coarse = coarse_scores                    # per shard: f32 [Q, n_s]
        self.sweeps = []

    def quantize_rows_e4m3(self, x):
        return x, torch.ones(x.shape[0])

    def rank_topk_mxfp4(self, tq, q_scale, codes, scales, k, *, splits=0, below=None):
        s = int(codes[0, 0])                           # the stand-in image names its shard in its first code byte
        cut = None if below is None else (below[0].numpy(), below[1].numpy())
        sc, ro = ref.top_lists(self.coarse[s], k, cut)
        return torch.from_numpy(sc), torch.from_numpy(ro)

    def topk_fold(self, run, incoming, shard, reset=False):
        Q, k = run[0].shape
        for q in range(Q):
            lists = [] if reset else [(run[0][q].numpy().copy(), run[2][q].numpy().copy(), run[1][q].numpy().copy())]
            sc = np.concatenate([l[0] for l in lists] + [incoming[0][q].numpy()]).astype(np.float64)
            sh = np.concatenate([l[2] for l in lists] + [np.full(incoming[0].shape[1], shard)])
            ro = np.concatenate([l[1] for l in lists] + [incoming[1][q].numpy()]).astype(np.int64)
            sc[ro == ref.EMPTY_ROW] = -np.inf
            sh[ro == ref.EMPTY_ROW] = ref.EMPTY_ROW
            order = np.lexsort((ro, sh, -sc))[:k]
            run[0][q], run[1][q], run[2][q] = (torch.from_numpy(a[order].astype(t)) for a, t in ((sc, np.float32), (sh, np.int32), (ro, np.int32)))
        return run

    def rank_topk(self, tq, vn, pair, k, *, splits=0):
        self.sweeps.append(vn.shape[0])
        sc, ro = ref.top_lists((tq.double() @ vn.double().T).float().numpy(), k)
        return None, None, torch.from_numpy(sc), torch.from_numpy(ro)


def _cpu_index(rows, seed=0):
    g = torch.Generator().manual_seed(seed)
    parts = []
    for s, n in enumerate(rows):
        feat = torch.randint(-8, 9, (n, 512), generator=g).float() / 16           # exact in f32 products and sums
        parts.append(srch.VideoIndex(feat, [0, n // 2, n], [f"s{s}a", f"s{s}b"]))
    return srch.ShardedIndex(parts)


def _cpu_image(rows):
    parts = []
    for s, n in enumerate(rows):
        codes = torch.zeros(n, 256, dtype=torch.uint8)
        codes[:, 0] = s
        parts.append((codes, torch.zeros(n, 16, dtype=torch.uint8)))
    return srch.CoarseImage(parts)


@pytest.mark.parametrize("pool", (7, 32, 45))
def test_candidate_union_and_back_mapping_over_a_stand_in(pool):
    rows = (50, 1, 80)
    index, image = _cpu_index(rows), _cpu_image(rows)
    g = torch.Generator().manual_seed(9)
    Q, k = 6, 5
    tq = torch.randint(-8, 9, (Q, 512), generator=g).float() / 16
    exact = [(tq.double() @ sh.feat.double().T).float() for sh in index.shards]
    coarse = [(e + 0.3 * torch.randn(e.shape, generator=g)).round().numpy() for e in exact]      # rounded: ties across shards
    ops = _DenseOps(coarse)
    score, shard, row = c2f.search_coarse(index, image, tq, tq, k, pool, ops=ops)
    # the candidates: per query the pool best of the concatenated coarse scores in (score, shard, row) order == global row order
    base = np.concatenate([[0], np.cumsum(rows)])
    whole_c, whole_e = np.concatenate(coarse, 1), torch.cat(exact, 1).numpy()
    cand = np.unique(ref.top_lists(whole_c, pool)[1])
    assert image.stats["unique"] == len(cand) and ops.sweeps == [len(cand)] and image.stats["rounds"] == -(-pool // 32)
    want_s, want_at = ref.top_lists(whole_e[:, cand], k)
    want_rows = cand[want_at]
    assert np.array_equal(base[shard] + row, want_rows) and np.array_equal(score, want_s)
    # the always-guarantee: the scores are the exact ones, the order the exact order restricted to the candidates
    assert np.array_equal(score, np.take_along_axis(whole_e, want_rows, 1))
    hits = c2f.locate(index, score, shard, row)
    v, sec = index.locate(shard, row)
    assert hits[0][0] == (index.vids[v[0, 0]], int(sec[0, 0]), float(score[0, 0]))


def test_unique_candidates_drops_empty_slots_and_sorts_by_shard_then_row():
    keys = c2f.unique_candidates([[2, 0, 0], [1, 0, 0x7FFFFFFF]], [[5, 9, 3], [0, 9, 0x7FFFFFFF]])
    shard, row = c2f.split_keys(keys)
    assert shard.tolist() == [0, 0, 1, 2] and row.tolist() == [3, 9, 0, 5]


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_coarse_with_restrict_and_a_mismatched_image_raise():
    index = _cpu_index((10, 12))
    with pytest.raises(ValueError, match="restrict"):
        srch.search(index, None, None, ["a"], coarse=_cpu_image((10, 12)), restrict=index.restrict(videos=["s0a"]))
    with pytest.raises(ValueError, match="does not fit"):
        srch.search(index, None, None, ["a"], coarse=_cpu_image((10, 11)))
    with pytest.raises(ValueError, match="does not fit"):
        srch.search(index, None, None, ["a"], coarse=_cpu_image((22,)))


def test_image_files_round_trip(tmp_path):
    image = _cpu_image((3, 5))
    image.parts[1][1][2, 7] = 131
    image.save(tmp_path / "i.c4.npz")
    back = srch.CoarseImage.load(tmp_path / "i.c4.npz", device="cpu")
    assert back.rows == [3, 5] and all(torch.equal(a, b) for p, r in zip(image.parts, back.parts) for a, b in zip(p, r))
    assert back.nbytes() == 8 * 272


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    assert L.tan_version() >= 106
    assert L.tan_quantize_rows_mxfp4(None, _lib.TAN_F32, 4, 512, None, None, None) == -1
    assert L.tan_rank_topk_mxfp4(None, None, None, None, 1, 1, 512, 1, 0, None, None, None, None, None, None) == -1
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    f = C.cast(p, C.POINTER(C.c_float))
    i = C.cast(p, C.POINTER(C.c_int))
    good = dict(Q=1, N=4, Cw=512, k=2, splits=0, bs=None, br=None)
    def call(**kw):                                                                # noqa: E306
        a = {**good, **kw}
        return L.tan_rank_topk_mxfp4(p, f, p, p, a["Q"], a["N"], a["Cw"], a["k"], a["splits"], a["bs"], a["br"], f, i, p, None)
    assert call(k=0) == -1 and call(k=33) == -1 and call(k=5) == -1 and call(Cw=256) == -1 and call(splits=-1) == -1
    assert call(bs=f) == -1 and call(br=i) == -1                                   # a cutoff is both arrays or neither
    assert call(N=0) == -1 and call(Q=0) == -1 and call(N=1 << 31) == -1
    assert L.tan_rank_topk_mxfp4_ws_bytes(33, 200003, 32) == 256 * 33 * 32 * 8 and L.tan_rank_topk_mxfp4_ws_bytes(1, 65, 1) == 16
    assert L.tan_rank_topk_mxfp4_ws_bytes(0, 5, 1) == -1 and L.tan_rank_topk_mxfp4_ws_bytes(1, 5, 33) == -1


def test_command_line_options():
    a = srch.parse_args(["coarse", "--index", "I.npz", "--shard", "J.npz", "--host-resident", "--out", "I.c4.npz"])
    assert (a.cmd, a.index, a.shard, a.host_resident, a.out) == ("coarse", "I.npz", ["J.npz"], True, "I.c4.npz")
    base = ["query", "--checkpoint", "c", "--vocab", "v", "--index", "I.npz"]
    a = srch.parse_args(base + ["--coarse", "I.c4.npz", "--pool", "128", "eggs"])
    assert a.coarse == "I.c4.npz" and a.pool == 128
    for bad in (["--pool", "64", "eggs"], ["--coarse", "x", "--moments", "eggs"], ["--coarse", "x", "--only", "v", "eggs"],
                ["--coarse", "x", "--pool", "0", "eggs"], ["--rerank", "--pool", "33", "eggs"]):
        with pytest.raises(SystemExit):
            srch.parse_args(base + bad)
