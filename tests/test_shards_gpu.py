"""Sharded search on the GPU: tan_topk_fold against its numpy statement (shard_ref.py), and `search` / `search_moments` /
`search_sequences` over a `ShardedIndex` -- device- and host-resident -- against the same call over `VideoIndex.concat` of the shards.
Every comparison is `==` (scores by value or bit pattern): the sharded answer is the concatenated index's answer, not close to it.

Index rows are the exact-arithmetic rows of test_retrieve_gpu.py / test_retrieve_fp8_gpu.py (multiples of 1/16; small-integer e4m3
codes with power-of-two scales), videos are layout (d) of test_moments_gpu.py inside every shard, and shards hold 1, 63, 64, 65 and
4097 rows (a single row; one 64-row tile less one, exactly, plus one; many tiles), in this order and reversed.  One row -- built from
query 0's feature, so that it IS query 0's best row -- stands in the 63-row and in the 4097-row shard: the best score of query 0 is a
tie across a shard boundary, resolved by shard number."""
import functools

import numpy as np
import pytest
import torch

import shard_ref as ref
from test_moments_gpu import DT, FORMATS, _expected, _layout_d
from test_retrieve_fp8_gpu import _deq, _int_codes
from test_retrieve_gpu import _embed, _exact_rows, _gen, _model

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4097)
KS = (1, 10, 32)
QUERIES = [f"query {i}" for i in range(33)]
SEQUENCES = [QUERIES[:1], QUERIES[:3], QUERIES[:32]]                   # one step, three steps, 32 steps (the most a sequence holds)


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


# ------------------------------------------------------------------------------------------------------------ 1. the fold kernel
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_fold(lists, order, Q, k, n_aux, run=None):
    """Fold lists[s] for s in `order` into a POISONED run list (the first fold resets it) -- or go on from `run` -- and read it back."""
    ops = _ops()
    if run is None:
        first = True
        run = (torch.full((Q, k), float("nan"), device="cuda"), torch.full((Q, k), -777, dtype=torch.int32, device="cuda"),
               torch.full((Q, k), -777, dtype=torch.int32, device="cuda"),
               torch.full((n_aux, Q, k), -777, dtype=torch.int32, device="cuda") if n_aux else None)
    else:
        first = False
        run = tuple(_cuda(t) for t in run[:3]) + (_cuda(run[3]) if n_aux else None,)
    for n, s in enumerate(order):
        score, row, aux = lists[s]
        got = ops.topk_fold(run, (_cuda(score), _cuda(row), *[_cuda(aux[c]) for c in range(n_aux)]), s, reset=first and n == 0)
        assert got is run
    return tuple(t.cpu().numpy() for t in run[:3]) + (run[3].cpu().numpy() if n_aux else np.zeros((0, Q, k), np.int32),)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Q", (1, 5, 130))                             # Q = 5: a partly filled workgroup of four waves
def test_fold_kernel_equals_the_reference_in_any_shard_order(Q, k):
    for k_in in sorted({1, k // 2 or 1, k}):
        for n_aux in (0, 1, 3):
            for S in (1, 2, 5):
                lists = ref.make_lists(Q, k_in, n_aux, range(S), seed=Q * 100000 + k * 1000 + k_in * 10 + S)
                want = ref.best_of_all(lists, k)
                orders = [list(range(S))] + ([list(range(S))[::-1], list(np.random.default_rng(S + k).permutation(S))] if S > 1 else [])
                for order in orders:
                    got = _gpu_fold(lists, order, Q, k, n_aux)
                    assert ref.same(got, want), (k_in, n_aux, S, order)


@pytest.mark.parametrize("kind", ("all_equal", "sentinels"))
def test_fold_kernel_on_equal_scores_and_on_incoming_sentinels(kind):
    for Q, k, k_in, n_aux, S in ((130, 32, 32, 3, 5), (5, 10, 5, 1, 5), (5, 10, 10, 0, 2), (1, 1, 1, 3, 5)):
        lists = ref.make_lists(Q, k_in, n_aux, range(S), seed=77 + k, **{kind: True})
        want = ref.best_of_all(lists, k)
        if kind == "all_equal" and S * k_in >= k:                       # nothing but (shard, row) decides
            assert (want[0] == 0.5).all() and (np.diff(want[1].astype(np.int64) * 1000 + want[2], axis=1) > 0).all()
        if kind == "sentinels" and k_in > 1:
            assert any((lists[s][1] == ref.SENT).any() for s in lists)
        for order in (list(range(S)), list(range(S))[::-1], list(np.random.default_rng(3).permutation(S))):
            got = _gpu_fold(lists, order, Q, k, n_aux)
            assert ref.same(got, want), (kind, Q, k, order)
            assert not (got[0] == 7.0).any()                            # a sentinel slot's stray score never gets in


def test_fold_kernel_empty_slots_reset_and_continuation():
    Q, k, k_in, n_aux = 6, 10, 3, 3
    lists = ref.make_lists(Q, k_in, n_aux, range(4), seed=5)
    one = _gpu_fold(lists, [2], Q, k, n_aux)                            # three entries in ten slots, over a poisoned run list
    assert ref.same(one, ref.best_of_all({2: lists[2]}, k))
    assert (one[1][:, :3] == 2).all() and np.isneginf(one[0][:, 3:]).all() and (one[1][:, 3:] == ref.SENT).all()
    assert (one[2][:, 3:] == ref.SENT).all() and (one[3][:, :, 3:] == -1).all()
    more = _gpu_fold(lists, [0, 3, 1], Q, k, n_aux, run=one)            # going on from a list that was read back: no reset
    assert ref.same(more, ref.best_of_all(lists, k))
    again = _gpu_fold(lists, [0, 3, 1], Q, k, n_aux, run=one)
    assert ref.same(again, more)                                        # run-to-run identical
    ops = _ops()
    run = tuple(_cuda(t) for t in more)
    with pytest.raises(Exception):
        ops.topk_fold(run, (_cuda(lists[0][0]), _cuda(lists[0][1])), 0)                       # n_aux of the two sides differ
    with pytest.raises(Exception):
        ops.topk_fold(run, tuple(t.cpu() for t in (_cuda(lists[0][0]), _cuda(lists[0][1]))) + tuple(torch.from_numpy(lists[0][2])), 0)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- shards and queries
@functools.lru_cache(maxsize=None)
def _the_model():
    return _model()


def _exact_shard(fmt, n, seed):
    """(feat, scale or None, v_off) of one shard: exact rows, layout (d)"""
    if fmt != "e4m3":
        feat, scale = _exact_rows(n, seed, DT[fmt]), None
    else:
        x = torch.randint(-16, 9, (n, 512), generator=_gen(seed), device="cuda")
        x[:, 0] = 16
        feat = _int_codes(x)
        scale = torch.ldexp(torch.ones(n, device="cuda"), torch.randint(-6, 4, (n,), generator=_gen(seed + 1), device="cuda"))
    return feat, scale, (np.array([0, 1], dtype=np.int64) if n == 1 else _layout_d(n))


def _best_row_for(fmt, t):
    """An exact row that is the unit f32 feature t's best row by far: x = round(256 t), so <x, t> is about 256.  f32 / bf16: x / 16,
    score about 16 against a few units for a random row.  e4m3: codes 16 x at the largest scale 2^3, score about 2^15 against a
    few thousand (a random row's values reach 16 * 16 * 2^3)."""
    x = (t * 256).round().clamp(-16, 16)
    if fmt != "e4m3":
        return (x / 16).to(DT[fmt]), None
    return _int_codes(x.long()), torch.tensor(2.0 ** 3, device="cuda")


@functools.lru_cache(maxsize=None)
def _shards(fmt, reverse=False, sizes=SIZES):
    srch = _srch()
    sizes = sizes[::-1] if reverse else sizes
    parts = []
    for s, n in enumerate(sizes):
        feat, scale, v_off = _exact_shard(fmt, n, 300 + 10 * s)
        parts.append(srch.VideoIndex(feat, v_off, [f"s{s}_{j}" for j in range(len(v_off) - 1)], scale))
    if 63 in sizes and 4097 in sizes:
        probe = srch.VideoIndex(torch.zeros(1, 512, device="cuda"), [0, 1], ["x"])
        row, sc = _best_row_for(fmt, srch.query_features(probe, _the_model(), _embed, QUERIES[:1])[0])
        for n, at in ((63, 5), (4097, 2077)):
            parts[sizes.index(n)].feat[at] = row
            if sc is not None:
                parts[sizes.index(n)].scale[at] = sc
    return parts


def _all_searches(index, queries, sequences, k):
    srch, m = _srch(), _the_model()
    return (srch.search(index, m, _embed, queries, k=k), srch.search_moments(index, m, _embed, queries, k=k),
            srch.search_sequences(index, m, _embed, sequences, k=k))


# ------------------------------------------------------------------------------------- 2. sharded == concatenated, bit for bit
@pytest.mark.parametrize("reverse", (False, True), ids=("1-63-64-65-4097", "reversed"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded_searches_equal_the_concatenated_index(fmt, reverse):
    srch = _srch()
    parts = _shards(fmt, reverse)
    whole, sharded = srch.VideoIndex.concat(parts), srch.ShardedIndex(parts)
    assert len(sharded) == len(whole) == sum(SIZES) and sharded.vids == whole.vids and sharded.v_off.tolist() == whole.v_off.tolist()
    assert min(len(p.vids) for p in parts) == 1 and min(len(p) for p in parts) == 1        # fewer rows / videos than k = 10, 32
    for k in KS:
        for Q, seqs in ((1, SEQUENCES[1:2]), (33, SEQUENCES)):
            want = _all_searches(whole, QUERIES[:Q], seqs, k)
            got = _all_searches(sharded, QUERIES[:Q], seqs, k)
            for name, g, w in zip(("search", "search_moments", "search_sequences"), got, want):
                assert g == w, (name, k, Q)
            assert all(len(h) == k for res in got for h in res)
    # the tie across the shard boundary is there, and the lower shard wins it
    hits = srch.search(sharded, _the_model(), _embed, QUERIES[:1], k=2)[0]
    lo, hi = sorted((SIZES[::-1] if reverse else SIZES).index(n) for n in (63, 4097))
    assert hits[0][2] == hits[1][2] and hits[0][0].startswith(f"s{lo}_") and hits[1][0].startswith(f"s{hi}_")


@pytest.mark.parametrize("fmt", FORMATS)
def test_k_is_clamped_to_the_total(fmt):
    """Shards of 1, 3 and 2 rows, one video each: 6 rows, 3 videos -- fewer than k in all."""
    srch = _srch()
    parts = []
    for s, n in enumerate((1, 3, 2)):
        feat, scale, _ = _exact_shard(fmt, n, 900 + s)
        parts.append(srch.VideoIndex(feat, [0, n], [f"c{s}"], scale))
    whole, sharded = srch.VideoIndex.concat(parts), srch.ShardedIndex(parts)
    for k in (10, 32, 2):
        want = _all_searches(whole, QUERIES[:33], SEQUENCES, k)
        got = _all_searches(sharded, QUERIES[:33], SEQUENCES, k)
        assert got == want, k
        assert [len(res[0]) for res in got] == [min(k, 6), min(k, 3), min(k, 3)]


def _bits(hits):
    """A search's result with every score as its f32 bit pattern: 0.0 and -0.0 differ here"""
    if isinstance(hits, float):
        return int(np.float32(hits).view(np.int32))
    if isinstance(hits, (list, tuple)):
        items = [_bits(h) for h in hits]
        return type(hits)(*items) if hasattr(hits, "_fields") else type(hits)(items)       # a namedtuple takes its fields one by one
    return hits


@pytest.mark.parametrize("fmt", ("bf16", "e4m3"))
def test_one_shard_is_the_index_itself_bit_for_bit(fmt):
    """A `ShardedIndex` of ONE shard against that `VideoIndex`: the fold of a single list against no fold, shard-local against global
    numbering.  Videos of 1, 63, 64, 65 and 130 rows: the 64-row tile edge after row 63 is a video boundary, the later ones lie inside
    videos.  Exact rows (small integers over 16), so equal scores occur and the order among them is compared too."""
    srch, m = _srch(), _the_model()
    vlens = (1, 63, 64, 65, 130)
    feat, scale, _ = _exact_shard(fmt, sum(vlens), 700)
    index = srch.VideoIndex(feat, np.concatenate([[0], np.cumsum(vlens)]), [f"v{j}" for j in range(len(vlens))], scale)
    one = srch.ShardedIndex([index])
    queries, sequences, k = QUERIES[:5], [QUERIES[:1], QUERIES[:3]], 3
    for name, call in (("search", srch.search), ("search_moments", srch.search_moments)):
        got, want = call(one, m, _embed, queries, k=k), call(index, m, _embed, queries, k=k)
        assert _bits(got) == _bits(want) and [len(h) for h in got] == [k] * 5, name
    got, want = (srch.search_sequences(ix, m, _embed, sequences, k=k) for ix in (one, index))
    assert _bits(got) == _bits(want) and [len(h.seconds) for h in got[1]] == [3] * k
    got, want = (srch.annotate(ix, m, _embed, QUERIES[:7], k=2) for ix in (one, index))
    assert got.label.shape == (sum(vlens), 2) and torch.equal(got.label, want.label)
    assert torch.equal(got.score.view(torch.int32), want.score.view(torch.int32))
    assert got.vids == want.vids and got.v_off.tolist() == want.v_off.tolist() and got.labels == want.labels
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. an independent reference
class _Identity:
    """A model whose text feature is the embedding itself: exact queries reach the sweeps"""
    @staticmethod
    def get_textual_feature(x):
        return x


@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded_search_and_moments_against_the_integer_dot_product(fmt):
    srch = _srch()
    parts = _shards(fmt)
    whole, sharded = srch.VideoIndex.concat(parts), srch.ShardedIndex(parts)
    Q, k = 9, 10
    # unit rows that are exact: 256 entries of +-1/16, the rest 0 (norm^2 = 256 / 256)
    sign = torch.randint(0, 2, (Q, 512), generator=_gen(41), device="cuda") * 2 - 1
    on = torch.stack([torch.randperm(512, generator=_gen(50 + q), device="cuda") < 256 for q in range(Q)])
    exact = (sign * on).float() / 16
    embed = lambda strs: exact[[int(s) for s in strs]]                                     # noqa: E731
    queries = [str(q) for q in range(Q)]
    tq = srch.query_features(sharded, _Identity, embed, queries)
    a = _deq(*tq) if fmt == "e4m3" else tq.double()
    assert torch.equal(a, exact.double())                                                  # the queries arrive exact
    b = _deq(whole.feat, whole.scale) if fmt == "e4m3" else whole.feat.double()
    S = a @ b.T                                                                            # exact in fp64, and in the f32 sweeps
    assert torch.equal(S.float().double(), S)
    rows = torch.sort(S, dim=1, descending=True, stable=True).indices[:, :k]
    v, sec = whole.locate(rows.cpu().numpy())
    want = [[(whole.vids[v[q, i]], int(sec[q, i]), float(S[q, rows[q, i]])) for i in range(k)] for q in range(Q)]
    assert srch.search(sharded, _Identity, embed, queries, k=k) == want
    vmax, vrow, order = (t.cpu().numpy() for t in _expected(S, whole.v_off, k))
    got = srch.search_moments(sharded, _Identity, embed, queries, k=k, width=0.0)
    for q in range(Q):
        for i, h in enumerate(got[q]):
            vnum = int(order[q, i])
            assert (h.vid, h.second, h.score) == (whole.vids[vnum], int(vrow[q, i] - whole.v_off[vnum]), float(vmax[q, i])), (q, i)
            assert 0 <= h.start <= h.second <= h.end < whole.v_off[vnum + 1] - whole.v_off[vnum]
            s_row = S[q, whole.v_off[vnum]:whole.v_off[vnum + 1]]                         # width 0: the run of rows equal to the peak
            assert bool((s_row[h.start:h.end + 1] == s_row[h.second]).all())
            assert (h.start == 0 or s_row[h.start - 1] < s_row[h.second]) and (h.end + 1 == len(s_row) or s_row[h.end + 1] < s_row[h.second])


# ------------------------------------------------------------------------------------------- 4. host-resident == device-resident
def _pinned(parts):
    srch = _srch()
    return [srch.VideoIndex(p.feat.cpu().pin_memory(), p.v_off, p.vids, None if p.scale is None else p.scale.cpu().pin_memory())
            for p in parts]


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_resident_equals_device_resident(fmt, tmp_path):
    srch, m = _srch(), _the_model()
    parts = _shards(fmt)
    dev = srch.ShardedIndex(parts, resident="device")
    host = srch.ShardedIndex(_pinned(parts), resident="host")
    assert host.resident == "host" and host.device.type == "cuda" and not host.shards[0].feat.is_cuda and len(host) == len(dev)
    k, queries = 10, QUERIES[:33]
    want = _all_searches(dev, queries, SEQUENCES, k)
    assert srch.search(host, m, _embed, queries, k=k) == want[0]
    assert srch.search(host, m, _embed, queries, k=k) == want[0]                           # the slots again, in a second call
    slots = [t.data_ptr() for t, _ in host._slots]
    assert host._slots[0][0].shape[0] == 4097                                              # sized to the largest shard, once
    assert srch.search_moments(host, m, _embed, queries, k=k) == want[1]
    assert srch.search_moments(host, m, _embed, queries, k=k) == want[1]
    assert srch.search_sequences(host, m, _embed, SEQUENCES, k=k) == want[2]               # phase 2 visits a subset of the shards
    assert srch.search_sequences(host, m, _embed, SEQUENCES[:1], k=1) == srch.search_sequences(dev, m, _embed, SEQUENCES[:1], k=1)
    assert srch.search(host, m, _embed, queries, k=k) == want[0]                           # and a plain search is still right
    assert [t.data_ptr() for t, _ in host._slots] == slots
    views = host.shard_views()                                                             # an early exit leaves the object usable
    next(views)
    views.close()
    assert srch.search(host, m, _embed, queries, k=32) == srch.search(dev, m, _embed, queries, k=32)
    if fmt == "bf16":                                                                      # the files, as `query --host-resident` reads them
        paths = [str(tmp_path / f"w{s}.npz") for s in range(len(parts))]
        for p, path in zip(parts, paths):
            p.save(path)
        loaded = srch.ShardedIndex.load(paths, resident="host")
        assert all(sh.feat.is_pinned() for sh in loaded.shards)
        assert _all_searches(loaded, queries, SEQUENCES, k) == want
        assert _all_searches(srch.ShardedIndex.load(paths), queries, SEQUENCES, k) == want
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- 5. the command line
def test_cli_index_by_two_workers_then_merge_and_query_shards(tmp_path, capsys):
    """`index --worker-id` twice, `merge`, and `query --index w0 --shard w1 [--host-resident]` prints what `query --index merged`
    prints -- in process (`search.main`): starting an interpreter per command would cost more than everything else in this file."""
    from temporalalignnet_amd import search as srch, synth
    from temporalalignnet_amd.train import build_model, default_args
    from temporalalignnet_amd.word2vec_model import Word2VecModel
    paths = synth.write_htm_fixture(str(tmp_path / "htm"), synth.htm_fixture())
    vocab = synth.w2v_vocab(40)
    np.save(str(tmp_path / "s3d_dict.npy"), vocab)
    m = build_model(default_args(model="init", num_encoder_layers=1, num_decoder_layers=1), compute_dtype="bf16", language_model=None,
                    random_pos_start=0)
    sd = m.state_dict()
    for key, v in synth.make_params(31, 1, 1, False).items():
        sd[key].copy_(torch.from_numpy(v))
    m.bert = Word2VecModel(num_embeddings=len(vocab) + 1, compute_dtype="bf16")
    for key, v in synth.w2v_params(32, len(vocab) + 1).items():
        m.bert.state_dict()[key].copy_(torch.from_numpy(v))
    ckpt = str(tmp_path / "ckpt.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 3}, ckpt)
    common = ["--checkpoint", ckpt, "--vocab", str(tmp_path / "s3d_dict.npy")]

    def run(*args):
        capsys.readouterr()
        assert srch.main(list(args)) == 0
        return capsys.readouterr().out

    files = [str(tmp_path / f"w{i}.npz") for i in range(2)]
    for i, f in enumerate(files):
        run("index", *common, "--feature-dir", paths["features"], "--asr-json", paths["asr"], "--vlen-csv", paths["vlen"], "--out", f,
            "--worker-id", str(i), "--num-workers", "2")
    merged = str(tmp_path / "all.npz")
    run("merge", "--out", merged, *files)
    parts, whole = [srch.VideoIndex.load(f) for f in files], srch.VideoIndex.load(merged)
    assert len(whole.vids) == 10 and whole.vids == parts[0].vids + parts[1].vids and min(len(p.vids) for p in parts) >= 1
    assert torch.equal(whole.feat, torch.cat([p.feat for p in parts]))
    sentences = ["stir the eggs", "w3 w7 w11", "w1 w2"]
    sharded = ["--index", files[0], "--shard", files[1]]
    for mode, more in (("--moments", sharded), ("--sequence", ["--index", merged, "--host-resident"])):      # one file, streamed, is a use too
        want = run("query", *common, "--index", merged, "-k", "4", mode, *sentences)
        assert len(want.splitlines()) == (4 if mode == "--sequence" else 12)
        assert run("query", *common, *sharded, "-k", "4", mode, *sentences) == want, mode
        assert run("query", *common, *more, "-k", "4", mode, *sentences) == want, mode
    want = run("query", *common, "--index", merged, "-k", "4", *sentences)
    assert len(want.splitlines()) == 12
    assert run("query", *common, *sharded, "-k", "4", *sentences) == want
    assert run("query", *common, *sharded, "--host-resident", "-k", "4", *sentences) == want


# ---------------------------------------------------------------------------------------------------------------------- 6. errors
def test_errors():
    srch, m = _srch(), _the_model()
    parts = _shards("bf16")
    with pytest.raises(ValueError, match="search_rerank: not built for a ShardedIndex; merge the shards"):
        srch.search_rerank(srch.ShardedIndex(parts), m, _embed, QUERIES[:2])
    unpinned = [srch.VideoIndex(p.feat.cpu(), p.v_off, p.vids) for p in parts]
    with pytest.raises(ValueError, match="pinned"):
        srch.ShardedIndex(unpinned, resident="host")
    with pytest.raises(ValueError, match="pinned"):
        srch.ShardedIndex(parts, resident="host")                                          # device rows are not host rows either
    host = srch.ShardedIndex(_pinned(parts), resident="host")
    host.shards[3].feat = host.shards[3].feat.clone()                                      # swapped for pageable memory afterwards
    with pytest.raises(ValueError, match="pinned"):
        srch.search(host, m, _embed, QUERIES[:2], k=3)
    with pytest.raises(ValueError):
        srch.ShardedIndex([parts[0], srch.VideoIndex(parts[1].feat.float(), parts[1].v_off, parts[1].vids)])
    with pytest.raises(ValueError):
        srch.search(srch.ShardedIndex(parts), m, _embed, QUERIES[:2], k=33)
    torch.cuda.synchronize()
