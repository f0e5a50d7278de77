"""Step discovery without a GPU: the numpy reference (cluster_ref.py) against brute force on tiny inputs, the entry points' and
`discover_steps`' argument checks, `StepClusters.save` / `load`, and the command line's parsing."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import cluster_ref as ref


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------- the reference
def test_fixed_point_image_is_round_to_nearest_even_of_the_exact_product():
    v = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 2.0 ** -23, -2.0 ** -23, 2.0 ** -30, 2.0 ** -31, 3 * 2.0 ** -31, -3 * 2.0 ** -31,
                  5 * 2.0 ** -31, 2.0 ** -32, 0.1, -0.3, 1e-12, np.float32(1) - np.float32(2.0 ** -24)], dtype=np.float32)
    got = ref.fixed_point(v)
    for x, q in zip(v.tolist(), got.tolist()):
        assert q == round(Fraction(x) * 2 ** 30)                       # Python rounds an exact fraction half to even
    assert got[:7].tolist() == [0, 2 ** 30, -2 ** 30, 2 ** 31, -2 ** 31, 128, -128]
    assert got[7:13].tolist() == [1, 0, 2, -2, 2, 0]                   # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 0.25 -> 0
    bf16 = torch.randn(4096).bfloat16().float().numpy()                # every bf16 value of magnitude >= 2^-23 is exact
    bf16 = bf16[np.abs(bf16) >= 2.0 ** -23]
    assert (ref.fixed_point(bf16).astype(np.float64) == bf16.astype(np.float64) * 2 ** 30).all()


def test_accumulate_equals_a_loop_over_python_integers():
    rng = np.random.default_rng(0)
    N, K = 23, 5
    rows = _unit(rng.standard_normal((N, 512))).astype(np.float32)
    assign = rng.integers(-1, K + 1, N)                                 # -1 and K are skipped
    assert (assign == -1).any() and (assign == K).any()
    want = [[0] * 512 for _ in range(K)]
    for n in range(N):
        if 0 <= assign[n] < K:
            for j in range(512):
                want[assign[n]][j] += round(Fraction(float(rows[n, j])) * 2 ** 30)
    got = ref.accumulate(rows, assign, K)
    assert got.dtype == np.int64 and got.tolist() == want
    again = ref.accumulate(rows[:10], assign[:10], K)                   # adding in two parts is adding at once
    assert (ref.accumulate(rows[10:], assign[10:], K, again) == got).all()
    perm = rng.permutation(N)
    assert (ref.accumulate(rows[perm], assign[perm], K) == got).all()


def test_centroids_are_the_normalised_means_and_empty_clusters_keep_theirs():
    rng = np.random.default_rng(1)
    N, K = 40, 4
    rows = _unit(rng.standard_normal((N, 512))).astype(np.float32)
    assign = rng.integers(0, 2, N)                                      # clusters 0 and 1; 2 stays empty; 3 cancels
    rows = np.concatenate([rows, rows[:1], -rows[:1]])
    assign = np.concatenate([assign, [3, 3]])
    prev = _unit(rng.standard_normal((K, 512))).astype(np.float32)
    cent, cohesion = ref.update(rows, assign, prev)
    for c in (0, 1):
        mean = rows[assign == c].astype(np.float64).sum(0)
        assert np.abs(cent[c] - mean / np.linalg.norm(mean)).max() < 1e-6
        assert abs(cohesion[c] - np.linalg.norm(mean) / (assign == c).sum()) < 1e-6 and 0 < cohesion[c] <= 1
        assert abs(np.linalg.norm(cent[c].astype(np.float64)) - 1) < 1e-6
    assert (cent[2:].view(np.int32) == prev[2:].view(np.int32)).all() and cohesion[2:].tolist() == [0, 0]
    one = ref.update(np.repeat(rows[:1], 7, 0), np.zeros(7, dtype=np.int64), prev[:1])
    assert np.abs(one[0][0] - rows[0]).max() < 1e-6 and abs(one[1][0] - 1) < 1e-6        # identical rows: cohesion 1


def test_lloyd_reference_equals_a_plain_fp64_k_means_on_separated_groups():
    rng = np.random.default_rng(2)
    dirs = _unit(rng.standard_normal((3, 512)))
    group = rng.integers(0, 3, 60)
    rows = _unit(dirs[group] + 0.3 * _unit(rng.standard_normal((60, 512)))).astype(np.float32)
    init = rows[[int(np.flatnonzero(group == g)[0]) for g in range(3)]]
    out = ref.lloyd(rows, lambda c: c.astype(np.float64), init, 10)
    cent = init.astype(np.float64)
    for _ in range(10):                                                 # brute force: exact means, renormalised
        assign = (rows.astype(np.float64) @ cent.T).argmax(1)
        cent = _unit(np.stack([rows[assign == c].astype(np.float64).sum(0) for c in range(3)]))
    assert (out["assign"] == assign).all() and (assign == group).all() and out["sizes"].tolist() == np.bincount(group).tolist()
    assert np.abs(out["centroids"] - cent).max() < 1e-6
    assert out["moved"][0] == 60 and out["moved"][-1] == 0 and len(out["moved"]) < 10 and min(out["margin"]) > 0.1


# ------------------------------------------------------------------------------------------------------- the C entry points
def test_entry_points_reject_bad_arguments_without_a_device():
    from temporalalignnet_amd import _lib, ops
    L = _lib.lib()
    assert L.tan_version() >= 105 and L.tan_cluster_slab_rows() == ops.CLUSTER_SLAB_ROWS == 256
    p = 4096                                                            # a non-NULL, aligned address: every call is refused before use
    assert L.tan_cluster_accumulate(None, 1, 8, 512, p, p, 2, p, None) == -1
    assert L.tan_cluster_accumulate(p, 1, 8, 512, None, p, 2, p, None) == -1
    assert L.tan_cluster_accumulate(p, 1, 8, 512, p, None, 2, p, None) == -1
    assert L.tan_cluster_accumulate(p, 1, 8, 512, p, p, 2, None, None) == -1
    assert L.tan_cluster_accumulate(p, 1, 8, 256, p, p, 2, p, None) == -1        # another width
    assert L.tan_cluster_accumulate(p, 2, 8, 512, p, p, 2, p, None) == -1        # an unknown dtype
    assert L.tan_cluster_accumulate(p, 1, 0, 512, p, p, 2, p, None) == -1
    assert L.tan_cluster_accumulate(p, 1, 1 << 31, 512, p, p, 2, p, None) == -1
    assert L.tan_cluster_accumulate(p, 1, 8, 512, p, p, 0, p, None) == -1
    assert L.tan_cluster_accumulate(p + 8, 1, 8, 512, p, p, 2, p, None) == -1    # rows are 16-byte aligned
    assert L.tan_cluster_accumulate_e4m3(p, None, 8, 512, p, p, 2, p, None) == -1
    assert L.tan_cluster_accumulate_e4m3(p, p, 8, 384, p, p, 2, p, None) == -1
    assert L.tan_cluster_centroids(None, p, p, 2, 512, p, p, None) == -1
    assert L.tan_cluster_centroids(p, p, p, 2, 512, p, None, None) == -1
    assert L.tan_cluster_centroids(p, p, p, 0, 512, p, p, None) == -1
    assert L.tan_cluster_centroids(p, p, p, 2, 64, p, p, None) == -1


def test_ops_wrappers_check_their_arguments_before_any_launch():
    from temporalalignnet_amd import ops
    vn, a, o, s = torch.zeros(8, 512), torch.zeros(8, dtype=torch.int32), torch.arange(8, dtype=torch.int32), torch.zeros(2, 512, dtype=torch.int64)
    for bad in (dict(vn=torch.zeros(8, 256)), dict(vn=torch.zeros(8, 512)[:, ::1].t().contiguous().t()), dict(assign=a.long()),
                dict(order=o[:7]), dict(sums=s.int()), dict(sums=torch.zeros(2, 256, dtype=torch.int64)), dict(v_scale=torch.ones(8)),
                dict(vn=torch.zeros(8, 512, dtype=torch.uint8))):
        kw = dict(vn=vn, assign=a, order=o, sums=s)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.cluster_accumulate(**kw)
    with pytest.raises(TypeError):
        ops.cluster_accumulate(vn.half(), a, o, s)
    c, p = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 512)
    for args, kw in (((s.int(), c, p), {}), ((s, c.long(), p), {}), ((s, c, p[:1]), {}), ((s, c, p.double()), {}),
                     ((s, c, p), dict(out=(p, torch.zeros(3)))), ((s, c, p), dict(out=(p.bfloat16(), torch.zeros(2))))):
        with pytest.raises(ValueError):
            ops.cluster_centroids(*args, **kw)


# ------------------------------------------------------------------------------------------------------------ discover_steps
def _cpu_index(n=10):
    from temporalalignnet_amd import search
    return search.VideoIndex(torch.zeros(n, 512), [0, n // 2, n], ["a", "b"])


def test_discover_steps_refuses_k_out_of_range_and_bad_init():
    from temporalalignnet_amd import search
    idx = _cpu_index()
    for k in (0, -1, 11):
        with pytest.raises(ValueError, match="k must lie"):
            search.discover_steps(idx, k)
    big = search.VideoIndex(torch.zeros(search.MAX_CLUSTERS + 2, 512, dtype=torch.bfloat16), [0, search.MAX_CLUSTERS + 2], ["a"])
    with pytest.raises(ValueError, match="k must lie"):
        search.discover_steps(big, search.MAX_CLUSTERS + 1)
    with pytest.raises(ValueError, match="iters"):
        search.discover_steps(idx, 2, iters=0)
    for init in (torch.zeros(3, 512), torch.zeros(2, 256), torch.zeros(2, 512, dtype=torch.float64), torch.zeros(2, 512).bfloat16(),
                 [0, 1, 2], [[0, 1]], [0.0, 1.0], "ab", np.array([0, 10]), np.array([-1, 3]), torch.tensor([0, 10])):
        with pytest.raises(ValueError, match="init"):
            search.discover_steps(idx, 2, init=init)


def test_step_clusters_save_and_load_round_trip(tmp_path):
    from temporalalignnet_amd import search
    rng = np.random.default_rng(3)
    K, N = 3, 10
    c = search.StepClusters(torch.from_numpy(_unit(rng.standard_normal((K, 512))).astype(np.float32)),
                            torch.from_numpy(rng.integers(0, K, N).astype(np.int32)), torch.from_numpy(rng.random(N).astype(np.float32)),
                            [4, 6, 0], [0.5, 0.25, 0.0], [10, 3, 0], [0.1, 0.2, 0.3], [0, 4, 10], ["a", "b:c"])
    path = str(tmp_path / "clusters.npz")
    c.save(path)
    d = search.StepClusters.load(path, device="cpu")
    assert len(d) == K and torch.equal(d.centroids, c.centroids) and torch.equal(d.assign, c.assign) and torch.equal(d.score, c.score)
    assert d.assign.dtype == torch.int32 and d.sizes.tolist() == [4, 6, 0] and d.cohesion.tolist() == [0.5, 0.25, 0.0]
    assert d.moved == [10, 3, 0] and d.objective == [0.1, 0.2, 0.3] and d.v_off.tolist() == [0, 4, 10] and d.vids == ["a", "b:c"]
    assert d.history is None and d.labels() == ["step 000", "step 001", "step 002"] and d.labels("xyz") == ["x", "y", "z"]
    with pytest.raises(ValueError):
        d.labels(["one"])
    with np.load(path, allow_pickle=False) as z:                        # plain arrays only
        assert sorted(z.files) == ["assign", "centroids", "cohesion", "moved", "objective", "score", "sizes", "v_off", "vids"]
    with pytest.raises(ValueError, match="k must lie"):
        d.annotation(_cpu_index(), k=4)


# ------------------------------------------------------------------------------------------------------------ the command line
def test_cli_parses_discover_and_annotate_clusters():
    from temporalalignnet_amd import search
    a = search.parse_args(["discover", "--index", "i.npz", "-k", "64", "--out", "c.npz"])
    assert (a.cmd, a.k, a.iters, a.seed, a.exemplars, a.segments, a.labels, a.checkpoint, a.shard, a.host_resident) == \
        ("discover", 64, 10, 0, None, None, None, None, None, False)
    a = search.parse_args(["discover", "--index", "i.npz", "--shard", "j.npz", "--host-resident", "-k", "8", "--iters", "3", "--seed", "5",
                           "--out", "c.npz", "--exemplars", "3", "--segments", "s.csv", "--threshold", "0.25", "--min-len", "2",
                           "--smooth", "0.1", "--labels", "l.txt", "--checkpoint", "c.pth", "--vocab", "v.npy"])
    assert (a.shard, a.host_resident, a.k, a.iters, a.seed, a.exemplars) == (["j.npz"], True, 8, 3, 5, 3)
    assert (a.segments, a.threshold, a.min_len, a.smooth, a.labels, a.checkpoint, a.vocab) == ("s.csv", 0.25, 2, 0.1, "l.txt", "c.pth", "v.npy")
    base = ["discover", "--index", "i.npz", "--out", "c.npz"]
    for bad in (["-k", "0"], ["-k", "16385"], [], ["-k", "4", "--iters", "0"], ["-k", "4", "--exemplars", "33"],
                ["-k", "4", "--threshold", "0.5"], ["-k", "4", "--min-len", "2"], ["-k", "4", "--segments", "s.csv", "--smooth", "0.1"],
                ["-k", "4", "--segments", "s.csv", "--smooth", "-1", "--threshold", "0.5"], ["-k", "4", "--segments", "s.csv", "--min-len", "0"],
                ["-k", "4", "--labels", "l.txt"], ["-k", "4", "--checkpoint", "c.pth", "--vocab", "v.npy"]):
        with pytest.raises(SystemExit) as e:
            search.parse_args(base + bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        search.parse_args(["discover", "-k", "4", "--out", "c.npz"])            # no index
    a = search.parse_args(["annotate", "--index", "i.npz", "--clusters", "c.npz", "--out", "o.csv", "-k", "5", "--threshold", "0.5",
                           "--smooth", "0.1"])
    assert (a.clusters, a.labels, a.checkpoint, a.vocab, a.k, a.smooth) == ("c.npz", None, None, None, 5, 0.1)
    a = search.parse_args(["annotate", "--checkpoint", "c", "--vocab", "v", "--index", "i.npz", "--labels", "l.txt", "--out", "o.csv"])
    assert (a.labels, a.clusters, a.k, a.dtype, a.model) == ("l.txt", None, 1, "bf16", "init")        # as before
    for bad in (["--index", "i.npz", "--out", "o.csv"], ["--index", "i.npz", "--labels", "l.txt", "--out", "o.csv"],
                ["--index", "i.npz", "--labels", "l.txt", "--checkpoint", "c", "--out", "o.csv"],
                ["--index", "i.npz", "--labels", "l.txt", "--clusters", "c.npz", "--checkpoint", "c", "--vocab", "v", "--out", "o.csv"]):
        with pytest.raises(SystemExit) as e:
            search.parse_args(["annotate"] + bad)
        assert e.value.code == 2
