"""Step discovery on the GPU: tan_cluster_accumulate / _e4m3 and tan_cluster_centroids against the numpy restatement
(cluster_ref.py) with `==`, `search.discover_steps` one pass at a time and as a whole trajectory, on a `VideoIndex` and on device-
and host-resident `ShardedIndex`es, and what is built on it (`StepClusters.annotation`, `exemplars`, the command line).

The sums are integers, so they are compared exactly whatever the order of the rows; the centroid arithmetic is float32 operation by
operation, so it is compared exactly too.  Only the ASSIGNMENT comes from a sweep with rounding (`tan_label_topk`): the
per-pass test checks that every pass's own assignment is valid within the sweep's error bound (EPS of test_annotate_gpu.py; for
e4m3 the bound of test_moments_gpu._stored) and that the update is exact GIVEN that assignment; the trajectory test uses planted,
well-separated groups, where the margins (asserted) put every assignment out of the rounding's reach.
R = ops.CLUSTER_SLAB_ROWS = 256 positions per wave: N runs over 1, R - 1, R, R + 1 and 3 R + 17."""
import functools

import numpy as np
import pytest
import torch

import cluster_ref as ref
import label_ref
from temporalalignnet_amd.ops import CLUSTER_SLAB_ROWS as R
from test_moments_gpu import FORMATS
from test_retrieve_fp8_gpu import ACC_EPS, _deq
from test_retrieve_gpu import EPS

pytestmark = pytest.mark.gpu

NS = (1, R - 1, R, R + 1, 3 * R + 17)
KS = (1, 2, 65, 300)
N_BIG = 3 * R + 17


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _rows(fmt, x):
    """f32 values x [N, 512] (numpy) -> (vn: the rows stored in the format, v_scale or None, the stored rows' VALUES as f32 numpy)"""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    if fmt == "f32":
        return x, None, x.cpu().numpy()
    if fmt == "bf16":
        vn = x.bfloat16()
        return vn, None, vn.float().cpu().numpy()
    codes, scale = _ops().quantize_rows_e4m3(x)
    return codes, scale, _deq(codes, scale).float().cpu().numpy()     # a code times a power of two: exact in f32


def _image(fmt, cent):
    """f32 centroids (numpy) -> fp64 numpy: their values as the sweep sees them (`search.centroid_image`)"""
    return _rows(fmt, cent)[2].astype(np.float64)


def _accumulate(vn, scale, assign, K, order=None, sums=None):
    assign = torch.as_tensor(np.asarray(assign), dtype=torch.int32).cuda()
    order = torch.argsort(assign, stable=True).int() if order is None else torch.as_tensor(np.asarray(order), dtype=torch.int32).cuda()
    sums = torch.zeros(K, 512, dtype=torch.int64, device="cuda") if sums is None else sums
    out = _ops().cluster_accumulate(vn, assign, order, sums, scale)
    assert out is sums
    return sums.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _random_case(fmt, N):
    rng = np.random.default_rng(100 + N)
    x = _unit(rng.standard_normal((N, 512)))
    x[::7] *= 2.0 ** -12                                               # small rows: the image rounds
    return _rows(fmt, x)


# --------------------------------------------------------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", NS)
def test_accumulate_equals_the_reference(N, fmt):
    vn, scale, values = _random_case(fmt, N)
    assert (values < 0).any() or N == 1
    rng = np.random.default_rng(N)
    cases = [(N, rng.permutation(N))]                                  # every row its own cluster
    for K in KS:
        cases.append((K, np.full(N, K - 1)))                           # one cluster: it spans every slab
        some = rng.choice(K, max(1, K // 2), replace=False)            # the others stay empty
        a = rng.choice(some, N)
        if N > 2:
            a[rng.integers(0, N, 3)] = -1                              # skipped
            a[rng.integers(0, N, 3)] = K
            a[0], a[N - 1] = K, -1
        cases.append((K, a))
    for K, a in cases:
        want = ref.accumulate(values, a, K)
        got = _accumulate(vn, scale, a, K)
        assert (got == want).all(), (K, int((got != want).sum()))
        assert want.any() or N <= 2


@pytest.mark.parametrize("fmt", FORMATS)
def test_accumulate_fixed_point_image(fmt):
    """negative values, 2^-23 (exact), ties and values that round to 0, +-2 (the contract's bound), and every element 1.0 over
    3 R + 17 rows: a column sum of 785 * 2^30, past 2^32"""
    special = np.array([1.0, -1.0, 2.0, -2.0, 2.0 ** -23, -2.0 ** -23, 2.0 ** -30, 2.0 ** -31, 3 * 2.0 ** -31, -5 * 2.0 ** -31, 2.0 ** -32,
                        0.0, 0.3125, -0.6875, 1.5 * 2.0 ** -20, 2.0 ** -40], dtype=np.float32)
    j = np.arange(512)
    x = np.stack([special[(j + n) % len(special)] for n in range(40)])
    x = np.concatenate([x, x * np.float32(2.0 ** -22), x[:, ::-1] * np.float32(2.0 ** -9)])
    vn, scale, values = _rows(fmt, x)
    if fmt != "e4m3":
        assert (values == x).all()                                     # all of them are bf16 values
    a = np.arange(len(x)) % 3
    want = ref.accumulate(values, a, 3)
    assert (_accumulate(vn, scale, a, 3) == want).all()
    assert (ref.fixed_point(values[:40]) == 0).any() and (np.abs(ref.fixed_point(values[:40])) == 2 ** 31).any()
    vn, scale, values = _rows(fmt, np.ones((N_BIG, 512)))
    got = _accumulate(vn, scale, np.zeros(N_BIG), 1)
    assert (got == N_BIG * 2 ** 30).all() and N_BIG * 2 ** 30 > 2 ** 32
    got = _accumulate(vn, scale, np.arange(N_BIG) % 2, 2)
    assert (got[0] == (N_BIG + 1) // 2 * 2 ** 30).all() and (got[1] == N_BIG // 2 * 2 ** 30).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_accumulate_is_the_same_for_every_order_and_every_split(fmt):
    N, K = N_BIG, 65
    vn, scale, values = _random_case(fmt, N)
    rng = np.random.default_rng(7)
    a = rng.integers(-1, K + 1, N)
    want = ref.accumulate(values, a, K)
    for order in (None, np.arange(N), rng.permutation(N), np.argsort(-a, kind="stable")):
        assert (_accumulate(vn, scale, a, K, order) == want).all()
    # three launches into one buffer (the shards of an index), on top of what the buffer held: the kernel ADDS
    sums = torch.full((K, 512), 7, dtype=torch.int64, device="cuda")
    for lo, hi in ((0, R - 1), (R - 1, R + 40), (R + 40, N)):
        _accumulate(vn[lo:hi], None if scale is None else scale[lo:hi], a[lo:hi], K, sums=sums)
    assert (sums.cpu().numpy() == want + 7).all()
    # an order that is no permutation: a position outside [0, N) is skipped, a row named twice counts twice
    order = np.arange(N)
    order[5], order[6], order[N - 1] = -1, N, 4
    keep = np.ones(N, dtype=bool)
    keep[[5, 6, N - 1]] = False
    twice = ref.accumulate(values[[4]], a[[4]], K, ref.accumulate(values[keep], a[keep], K))
    assert (_accumulate(vn, scale, a, K, order) == twice).all()


# --------------------------------------------------------------------------------------------------------------- 2. centroids
def test_centroids_equal_the_reference():
    ops = _ops()
    rng = np.random.default_rng(11)
    K, N = 70, 900                                                     # 70: the last workgroup holds two clusters of four
    rows = _unit(rng.standard_normal((N, 512))).astype(np.float32)
    rows[:300] = _unit(rows[:300] + 3 * rows[0])                       # a tight cluster next to loose ones
    a = rng.integers(4, K, N)
    a[:300] = 4
    rows[-2], a[-2:] = -rows[-1], 2                                    # cluster 2: two rows that cancel; 0, 1, 3: empty
    sums = ref.accumulate(rows, a, K)
    assert not sums[2].any() and not sums[[0, 1, 3]].any()
    sums[5] = rng.integers(-2 ** 52, 2 ** 52, 512)                     # sums beyond f32's 24 bits: the conversion rounds
    sums[6, :] = 0
    sums[6, 17] = 3                                                    # one tiny component
    counts = np.bincount(a, minlength=K)
    counts[1] = 9                                                      # rows counted, nothing summed: norm 0 keeps prev too
    prev = rng.standard_normal((K, 512)).astype(np.float32)
    want_c, want_h = ref.centroids(sums, counts, prev)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()                       # noqa: E731
    d_sums, d_counts, d_prev = dev(sums, torch.int64), dev(counts, torch.int32), dev(prev, torch.float32)
    cent, coh = ops.cluster_centroids(d_sums, d_counts, d_prev)
    assert (cent.cpu().numpy().view(np.int32) == want_c.view(np.int32)).all()
    assert (coh.cpu().numpy().view(np.int32) == want_h.view(np.int32)).all()
    assert (want_c[:4].view(np.int32) == prev[:4].view(np.int32)).all() and want_h[:4].tolist() == [0, 0, 0, 0]
    assert want_h[4] > 0.9 > want_h[7] > 0 and np.isfinite(want_c).all()
    # caller-owned outputs, cent being prev itself; nothing is written behind cluster K - 1
    whole = torch.full((K + 2, 512), 5.0, device="cuda")
    whole[:K] = d_prev
    hold = torch.full((K + 2,), 5.0, device="cuda")
    out = ops.cluster_centroids(d_sums, d_counts, whole[:K], out=(whole[:K], hold[:K]))
    assert out[0].data_ptr() == whole.data_ptr() and torch.equal(whole[:K], cent) and torch.equal(hold[:K], coh)
    assert (whole[K:] == 5.0).all() and (hold[K:] == 5.0).all()
    one = ops.cluster_centroids(d_sums[7:8].contiguous(), d_counts[7:8].contiguous(), d_prev[7:8].contiguous())       # K = 1
    assert torch.equal(one[0], cent[7:8]) and torch.equal(one[1], coh[7:8])


# ------------------------------------------------------------------------------------------------- 3. discover_steps, pass by pass
def _index(fmt, x, n_videos=9, seed=0):
    """(VideoIndex of the rows x in the format, the stored rows' values f32 numpy); video boundaries at random rows"""
    vn, scale, values = _rows(fmt, x)
    N = len(x)
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, N), n_videos - 1, replace=False)) if n_videos > 1 else []
    v_off = np.concatenate([[0], cuts, [N]]).astype(np.int64)
    return _srch().VideoIndex(vn, v_off, [f"v{i}" for i in range(n_videos)], scale), values


def _bound(fmt, rows64, image64):
    """[N, 1] fp64: the bound on the error of a sweep's score of these stored operands"""
    if fmt != "e4m3":
        return np.full((len(rows64), 1), EPS)
    return (ACC_EPS * (np.abs(rows64) @ np.abs(image64).T)).max(1, keepdims=True)


@pytest.mark.parametrize("fmt", FORMATS)
def test_discover_steps_every_pass_is_a_valid_assignment_and_an_exact_update(fmt):
    N, K, iters = N_BIG, 12, 4
    idx, values = _index(fmt, _unit(np.random.default_rng(21).standard_normal((N, 512))))
    found = _srch().discover_steps(idx, K, iters=iters, seed=3, history=True)
    assert 2 <= len(found.history) == len(found.moved) == len(found.objective) <= iters + 1 and found.moved[0] == N
    assert len(found.moved) == iters + 1 or found.moved[-1] == 0      # all the updates, or a pass that moved nothing
    assert all(m > 0 for m in found.moved[:-1])
    rows64 = values.astype(np.float64)
    init = np.sort(np.random.default_rng(3).choice(N, K, replace=False))
    start = found.history[0][1].cpu().numpy()
    assert np.abs(start - _unit(values[init].astype(np.float64))).max() < 1e-6          # the drawn rows, normalised
    for t, (assign, cent) in enumerate(found.history):
        assign, cent = assign.cpu().numpy().astype(np.int64), cent.cpu().numpy()
        image = _image(fmt, cent)
        S = rows64 @ image.T
        eps = _bound(fmt, rows64, image)
        own = np.take_along_axis(S, assign[:, None], 1)
        print(f"pass {t} {fmt}: moved {found.moved[t]}, objective {found.objective[t]:.6f}, worst shortfall "
              f"{float((S.max(1, keepdims=True) - own).max()):.3e} against 2 x {float(eps.max()):.3e}")
        assert assign.min() >= 0 and assign.max() < K
        assert (S.max(1, keepdims=True) - own <= 2 * eps).all()        # no other cluster scores more than twice the bound higher
        if t == len(found.history) - 1:
            score = found.score.cpu().numpy().astype(np.float64)[:, None]
            assert (np.abs(score - S.max(1, keepdims=True)) <= eps).all() and (np.abs(score - own) <= eps).all()
            assert abs(found.objective[t] - float(score.mean())) < 1e-12
            assert (found.assign.cpu().numpy() == assign).all() and (found.centroids.cpu().numpy() == cent).all()
            want_c, want_h = ref.update(values, assign, cent)
            assert found.sizes.tolist() == np.bincount(assign, minlength=K).tolist()
            assert (found.cohesion.view(np.int32) == want_h.view(np.int32)).all()
        else:
            nxt = found.history[t + 1][1].cpu().numpy()
            assert (nxt.view(np.int32) == ref.update(values, assign, cent)[0].view(np.int32)).all(), t
            assert found.moved[t + 1] == int((found.history[t + 1][0].cpu().numpy() != assign).sum())
    assert found.objective[-1] > found.objective[0] and found.vids == idx.vids and found.v_off.tolist() == idx.v_off.tolist()
    again = _srch().discover_steps(idx, K, iters=iters, seed=3)
    assert again.history is None and torch.equal(again.centroids, found.centroids) and torch.equal(again.assign, found.assign)
    assert torch.equal(again.score.view(torch.int32), found.score.view(torch.int32))


# --------------------------------------------------------------------------------------------- 4. the trajectory on planted groups
GROUPS = 7


def _planted(seed=5, N=N_BIG, noise=0.3):
    """(x f64 [N, 512], group [N]): rows = unit(direction + noise * unit noise) around GROUPS random unit directions"""
    rng = np.random.default_rng(seed)
    dirs = _unit(rng.standard_normal((GROUPS, 512)))
    group = rng.integers(0, GROUPS, N)
    group[:GROUPS] = np.arange(GROUPS)
    return _unit(dirs[group] + noise * _unit(rng.standard_normal((N, 512)))), group


def _planted_init(values, group):
    """one stored row per group, and one centroid opposite to the mean of all rows: nothing is ever assigned to it"""
    first = [int(np.flatnonzero(group == g)[0]) for g in range(GROUPS)]
    away = -_unit(values.astype(np.float64).mean(0))
    return np.concatenate([values[first], away[None].astype(np.float32)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_discover_steps_follows_the_reference_trajectory_on_planted_groups(fmt):
    x, group = _planted()
    idx, values = _index(fmt, x)
    init = _planted_init(values, group)
    iters = 10
    want = ref.lloyd(values, lambda c: _image(fmt, c), init, iters)
    bound = max(float(_bound(fmt, values.astype(np.float64), _image(fmt, init)).max()), EPS)
    print(f"planted {fmt}: reference margins {['%.3f' % m for m in want['margin']]}, moved {want['moved']}, 100 x bound {100 * bound:.3e}")
    assert min(want["margin"]) > 100 * bound                           # otherwise the INPUT is broken, not the kernels
    found = _srch().discover_steps(idx, GROUPS + 1, iters=iters, init=torch.from_numpy(init).cuda(), history=True)
    assert found.moved == want["moved"] and found.moved[-1] == 0 and len(found.moved) <= iters
    assert (found.assign.cpu().numpy() == want["assign"]).all() and found.sizes.tolist() == want["sizes"].tolist()
    assert (found.centroids.cpu().numpy().view(np.int32) == want["centroids"].view(np.int32)).all()
    assert (found.cohesion.view(np.int32) == want["cohesion"].view(np.int32)).all()
    assert (want["assign"] == group).all()                             # the planted groups, under their init rows' numbers
    assert found.sizes[GROUPS] == 0 and found.cohesion[GROUPS] == 0    # the opposite centroid: empty and unchanged
    assert (found.centroids[GROUPS].cpu().numpy().view(np.int32) == init[GROUPS].view(np.int32)).all()
    assert (found.cohesion[:GROUPS] > 0.9).all()
    last = _bound(fmt, values.astype(np.float64), _image(fmt, want["centroids"]))
    assert (np.abs(found.score.cpu().numpy() - want["score"])[:, None] <= last).all()


# ------------------------------------------------------------------------------------------------------------------ 5. sharded
@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_sharded_discovery_equals_concat_bit_for_bit(fmt):
    from test_shards_gpu import _pinned
    srch = _srch()
    x = _unit(np.random.default_rng(31).standard_normal((N_BIG, 512)))
    parts, lo = [], 0
    for s, n in enumerate((R + 1, 1, N_BIG - R - 2)):                  # a one-row shard in the middle
        parts.append(_index(fmt, x[lo:lo + n], n_videos=min(3, n), seed=s)[0])
        parts[-1].vids = [f"s{s}_{v}" for v in parts[-1].vids]
        lo += n
    whole = srch.VideoIndex.concat(parts)
    want = srch.discover_steps(whole, 12, iters=3, seed=1)
    for sharded in (srch.ShardedIndex(parts), srch.ShardedIndex(_pinned(parts), resident="host")):
        for _ in range(2):                                             # the host slots again, in a second call
            got = srch.discover_steps(sharded, 12, iters=3, seed=1)
            assert got.assign.is_cuda and torch.equal(got.assign, want.assign)
            assert torch.equal(got.score.view(torch.int32), want.score.view(torch.int32))
            assert torch.equal(got.centroids.view(torch.int32), want.centroids.view(torch.int32))
        assert got.moved == want.moved and got.sizes.tolist() == want.sizes.tolist() and got.vids == want.vids
        assert (got.cohesion.view(np.int32) == want.cohesion.view(np.int32)).all() and got.v_off.tolist() == want.v_off.tolist()
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- 6. composition
@functools.lru_cache(maxsize=None)
def _found(fmt):
    x, group = _planted(seed=9)
    idx, values = _index(fmt, x)
    return idx, values, _srch().discover_steps(idx, GROUPS, iters=5, seed=2)


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_annotation_segments_are_the_runs_of_the_final_assignment(fmt):
    idx, values, found = _found(fmt)
    ann = found.annotation(idx)
    assert torch.equal(ann.label[:, 0], found.assign) and torch.equal(ann.score[:, 0].view(torch.int32), found.score.view(torch.int32))
    assert ann.labels == [f"step {c:03d}" for c in range(GROUPS)] and ann.vids == idx.vids
    s0, l0 = found.score.cpu().numpy(), found.assign.cpu().numpy()
    threshold = float(np.median(s0))
    for min_len in (1, 2):
        want = label_ref.label_runs(s0, l0, idx.v_off, threshold, min_len)
        assert len(want) > 0 or min_len > 1
        assert ann.segments(threshold, min_len) == [
            (idx.vids[v], a - idx.v_off[v], b - idx.v_off[v], f"step {lab:03d}", pr - idx.v_off[v], ps) for v, a, b, lab, pr, ps in want]
    counts = ann.label_seconds(float("-inf"))
    assert [counts[f"step {c:03d}"] for c in range(GROUPS)] == found.sizes.tolist()
    names = [f"n{c}" for c in range(GROUPS)]
    top3 = found.annotation(idx, k=3, names=names)                     # k > 1 and names; `decode` takes such lists
    assert top3.labels == names and torch.equal(top3.label[:, 0], found.assign) and top3.decode(threshold, 0.05)[0].shape == (len(idx),)
    other, _ = _index("f32" if fmt == "bf16" else "bf16", _planted(seed=9)[0][:100], n_videos=2)       # another index, another format
    assert found.annotation(other).label.shape == (100, 1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_exemplars_are_the_best_rows_of_every_centroid(fmt):
    idx, values, found = _found(fmt)
    n = 3
    best = found.exemplars(idx, n)
    image = _image(fmt, found.centroids.cpu().numpy())
    S = image @ values.astype(np.float64).T                            # [K, N]
    eps = _bound(fmt, image, values.astype(np.float64))
    assert len(best) == GROUPS and all(len(b) == n for b in best)
    for c, hits in enumerate(best):
        rows = [int(idx.v_off[idx.vids.index(vid)]) + sec for vid, sec, _ in hits]
        assert len(set(rows)) == n and [h[2] for h in hits] == sorted((h[2] for h in hits), reverse=True)
        assert all(abs(sc - S[c, r]) <= eps[c, 0] for r, (_, _, sc) in zip(rows, hits))
        rest = np.delete(S[c], rows)
        assert rest.max() <= min(S[c, rows]) + 2 * eps[c, 0]           # no other row scores higher, within the bound
    with pytest.raises(ValueError):
        found.exemplars(idx, 0)


def test_cli_discover_then_annotate_clusters(tmp_path, capsys):
    """`discover` on a saved synthetic index (no checkpoint, no vocabulary), then `annotate --clusters` on a second index: the files
    the API gives, in process (`search.main`) as test_annotate_gpu.py runs the command line."""
    import io
    srch = _srch()
    x, group = _planted(seed=13)
    first, second = _index("bf16", x[:500], n_videos=5)[0], _index("bf16", x[500:], n_videos=4, seed=1)[0]
    p1, p2, out, seg = (str(tmp_path / n) for n in ("i1.npz", "i2.npz", "clusters.npz", "seg.csv"))
    first.save(p1)
    second.save(p2)
    want = srch.discover_steps(srch.VideoIndex.load(p1), GROUPS, iters=6, seed=4)
    threshold = float(want.score.median())
    capsys.readouterr()
    assert srch.main(["discover", "--index", p1, "-k", str(GROUPS), "--iters", "6", "--seed", "4", "--out", out, "--exemplars", "2",
                      "--segments", seg, f"--threshold={threshold!r}", "--min-len", "2"]) == 0
    printed = capsys.readouterr().out.splitlines()
    got = srch.StepClusters.load(out)
    assert torch.equal(got.centroids, want.centroids) and torch.equal(got.assign, want.assign) and got.moved == want.moved
    assert got.sizes.tolist() == want.sizes.tolist() and got.vids == first.vids
    ex = want.exemplars(first, 2)
    assert len(printed) == GROUPS
    for c, line in enumerate(printed):
        cells = line.split("\t")
        assert cells[:3] == [str(c), str(int(want.sizes[c])), f"{want.cohesion[c]:.6f}"]
        assert cells[3:] == [f"{vid}:{sec}:{score:.6f}" for vid, sec, score in ex[c]]
    buf = io.StringIO()
    srch.write_segments_csv(buf, want.annotation(first).segments(threshold, 2))
    assert open(seg).read() == buf.getvalue() and len(buf.getvalue().splitlines()) > 1
    # the same steps on a second index, device- and host-resident, plain and decoded
    for more in ((), ("--host-resident",)):
        ann_out = str(tmp_path / f"ann{len(more)}.csv")
        assert srch.main(["annotate", "--index", p2, "--clusters", out, "-k", "3", f"--threshold={threshold / 2!r}", "--smooth", "0.02",
                          "--out", ann_out, *more]) == 0                # half the median: a second gains far more than a change costs
        buf = io.StringIO()
        srch.write_segments_csv(buf, want.annotation(second, 3).segments(threshold / 2, 1, switch=0.02))
        assert open(ann_out).read() == buf.getvalue() and len(buf.getvalue().splitlines()) > 1
    assert srch.main(["annotate", "--index", p2, "--clusters", out, "-k", "9", "--out", str(tmp_path / "no.csv")]) == 2
    capsys.readouterr()
