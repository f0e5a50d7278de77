"""Coarse-to-fine search on the GPU: tan_quantize_rows_mxfp4, tan_rank_topk_mxfp4, `CoarseImage`, `search(..., coarse=)`.
The row format is the one include/tan_hip.h fixes; tests/coarse_ref.py restates it in numpy.

  * quantiser: codes and scale bytes compared with `==` against the reference, no exclusions.
  * sweep, exact arithmetic: index codes from the whole e2m1 table, block scales 2^-3 .. 2^3, integer queries from an asymmetric
    range with power-of-two row scales, Q != N.  Every term is a multiple of one power of two g and the sum of the terms' magnitudes
    is below 2^24 g (asserted on the host), so every partial sum in any order is exact in f32: rows, tie order and scores are
    compared with `==` against fp64 integer arithmetic.  One case gives each of a row's 16 blocks a different scale, a second
    plants a single nonzero element at every position 0..511 in turn: a permuted block, nibble or scale byte cannot pass both.
  * cutoff: 16 + 16 == 32 with duplicate rows (equal scores) across the cut; cutoff rows -1 and 0x7fffffff.
  * splits: the same lists for splits in {1, 7, 256}.
  * sweep, random unit rows: against the fp64 product of the dequantised operands with the e4m3 tests' per-score bound
        eps(q, n) = 512 * 2^-23 * sum_i |a_i b_i|
    which assumes the scaled MFMA accumulates no worse than an f32 truncation chain; the worst observed ratio is printed.
  * format error against the unquantised scores: printed, not asserted.
  * end to end: `search(..., coarse=image)` == `search(...)` on a `VideoIndex` (f32, bf16, e4m3) and a three-shard `ShardedIndex`
    (device- and host-resident) once the reference says the exact top k lie well inside the coarse top `pool`; with pool < k the
    returned entries are a subsequence of the uncoarsened list, scores bit for bit; a host-resident search stages U rows and
    allocates no shard slots.
"""
import functools

import numpy as np
import pytest
import torch

import coarse_ref as ref

pytestmark = pytest.mark.gpu

QS, NS, KS = (1, 33, 130), (1, 63, 65, 4097), (1, 10, 32)
SHAPES = [(Q, N) for Q in QS for N in NS] + [(33, 200003)]
ACC_EPS = 512 * 2.0 ** -23
INT_MAX = 0x7FFFFFFF


def _ops():
    from temporalalignnet_amd import ops
    return ops


def _srch():
    from temporalalignnet_amd import search
    return search


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _e4m3_rows(values, scale_exp):
    """integer (or any e4m3-exact) values [Q, 512] and per-row scale exponents -> (codes uint8 [Q, 512], q_scale f32 [Q]) on the device"""
    codes = torch.from_numpy(np.asarray(values, dtype=np.float32)).to(torch.float8_e4m3fn)
    assert np.array_equal(codes.float().numpy(), np.asarray(values, dtype=np.float32))
    return codes.view(torch.uint8).cuda().contiguous(), _dev(np.ldexp(1.0, np.asarray(scale_exp)).astype(np.float32))


def _host_e4m3(x):
    """tan_quantize_rows_e4m3's format on the host (tests/test_retrieve_fp8_gpu.py): (codes uint8 [n, 512], scale f32 [n])"""
    x = x.detach().float().cpu()
    amax = x.abs().amax(dim=1)
    m, e = torch.frexp(amax)
    s = torch.where(m <= 0.875, e - 9, e - 8).clamp(-126, 127)
    s = torch.where(amax == 0, torch.zeros_like(s), s)
    one = torch.ones_like(amax)
    return (x * torch.ldexp(one, -s)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), torch.ldexp(one, s).numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. quantiser
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def _quant_rows(n_rows, seed):
    """f32 rows: the special rows first (a zero row; a row with zero blocks; rows of table values, ties and their neighbours under
    several block scales; the m = 0.75 edge both ways; clamped scales), then rows over many binades"""
    rng = np.random.default_rng(seed)
    pool = list(ref.E2M1) + list(TIES)
    pool += [np.nextafter(np.float32(t), np.float32(9)) for t in TIES] + [np.nextafter(np.float32(t), np.float32(0)) for t in TIES]
    pool += [t + 2.0 ** -6 for t in TIES] + [t - 2.0 ** -6 for t in TIES]         # neighbours that bf16 holds too
    pool = np.asarray(pool, dtype=np.float32)
    rows = [np.zeros(512, dtype=np.float32)]
    r = rng.standard_normal(512).astype(np.float32)
    r[32:64] = 0
    r[480:] = 0
    r[100] = -0.0
    rows.append(r)
    for t in (-20, -3, 0, 5, 100, -120):                                          # block amax 6 * 2^t: s == t, the pool lands on the grid
        for _ in range(2):
            v = rng.choice(pool, 512) * rng.choice(np.float32([-1, 1]), 512)
            v = v.reshape(16, 32)
            v[:, 0] = 6.0
            rows.append((np.ldexp(v, t)).reshape(512).astype(np.float32))
    edge = rng.uniform(-0.4, 0.4, (16, 32)).astype(np.float32)                    # amax = 0.75 * 2^e exactly, one ulp above, and 0.5 * 2^e
    for b in range(16):
        edge[b, b] = (np.float32(0.75), np.nextafter(np.float32(0.75), np.float32(1)), np.float32(0.5),
                      np.nextafter(np.float32(0.5), np.float32(0)))[b % 4] * (-1) ** b
    rows.append(edge.reshape(512))
    for e in (-140, -127, -126, 120, 126):                                        # subnormal amax and the clamp; the top of the range
        rows.append(np.ldexp(rng.uniform(-1, 1, 512), e).astype(np.float32))
    rows = rows[:n_rows]
    while len(rows) < n_rows:
        e = rng.integers(-40, 40, (16, 1))
        rows.append(np.ldexp(rng.standard_normal((16, 32)), e).reshape(512).astype(np.float32))
    return np.stack(rows)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("n_rows", (1, 5, 257))
def test_quantiser_equals_the_reference(n_rows, dtype):
    x = torch.from_numpy(_quant_rows(n_rows, 3 + n_rows)).to(dtype).cuda()
    codes, scales = _ops().quantize_rows_mxfp4(x)
    want_c, want_s = ref.quantize(x.float().cpu().numpy())
    assert np.array_equal(scales.cpu().numpy(), want_s)
    assert np.array_equal(codes.cpu().numpy(), want_c)
    assert int(scales.max()) < 255


# ------------------------------------------------------------------------------------------------------- 2. sweep, exact arithmetic
@functools.lru_cache(maxsize=None)
def _exact_case(Q, N):
    """(device operands, exact scores f64 [Q, N]) of one shape; the second half of the index repeats the first: equal scores"""
    rng = np.random.default_rng(1000 * Q + N)
    codes = rng.integers(0, 256, (N, 256), dtype=np.uint8)
    scales = rng.integers(124, 131, (N, 16), dtype=np.uint8)                      # 2^-3 .. 2^3 per block
    if N > 1:
        codes[(N + 1) // 2:], scales[(N + 1) // 2:] = codes[:N // 2], scales[:N // 2]
    q_int = rng.integers(-3, 6, (Q, 512))                                         # asymmetric
    q_exp = rng.integers(-2, 3, Q)
    want, worst = ref.score_c_exact(q_int, np.ldexp(1.0, q_exp), codes, scales)
    assert worst < 2 ** 24                                                        # every partial sum is exact in f32
    tq, q_scale = _e4m3_rows(q_int, q_exp)
    return (tq, q_scale, _dev(codes), _dev(scales)), want


def _assert_lists(got, want_scores, k, below=None):
    top_s, top_r = (t.cpu().numpy() for t in got)
    want_s, want_r = ref.top_lists(want_scores, k, below)
    assert np.array_equal(top_r, want_r)
    assert np.array_equal(top_s, want_s)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Q,N", SHAPES)
def test_sweep_is_exact_on_integer_data(Q, N, k):
    args, want = _exact_case(Q, N)
    k = min(k, N)
    _assert_lists(_ops().rank_topk_mxfp4(*args, k), want, k)


def test_sweep_with_sixteen_different_block_scales_per_row():
    rng = np.random.default_rng(5)
    Q, N = 33, 130
    nib = rng.choice(np.array([0, 1, 2, 9, 10], dtype=np.uint8), (N, 512))        # 0, +-0.5, +-1
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    scales = np.stack([rng.permutation(16) for _ in range(N)]).astype(np.uint8) + 119     # 2^-8 .. 2^7, each once per row
    q_int, q_exp = rng.integers(-1, 3, (Q, 512)), rng.integers(-2, 3, Q)
    want, worst = ref.score_c_exact(q_int, np.ldexp(1.0, q_exp), codes, scales)
    assert worst < 2 ** 24
    tq, q_scale = _e4m3_rows(q_int, q_exp)
    _assert_lists(_ops().rank_topk_mxfp4(tq, q_scale, _dev(codes), _dev(scales), 32), want, 32)


def test_sweep_finds_a_single_element_at_every_position():
    rng = np.random.default_rng(6)
    Q, N = 33, 512
    nib = np.zeros((N, 512), dtype=np.uint8)
    nib[np.arange(N), np.arange(N)] = (1 + np.arange(N) % 7) | ((np.arange(N) // 7 % 2) << 3)
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    scales = rng.integers(124, 131, (N, 16), dtype=np.uint8)
    q_int, q_exp = rng.integers(-3, 6, (Q, 512)), rng.integers(-2, 3, Q)
    want, worst = ref.score_c_exact(q_int, np.ldexp(1.0, q_exp), codes, scales)
    assert worst < 2 ** 24
    tq, q_scale = _e4m3_rows(q_int, q_exp)
    _assert_lists(_ops().rank_topk_mxfp4(tq, q_scale, _dev(codes), _dev(scales), 32), want, 32)


# ------------------------------------------------------------------------------------------------------------ 3. cutoff, splits
def test_a_continued_list_equals_the_one_shot_list():
    ops = _ops()
    # every row three times (rows n, n + 1365, n + 2730; two rows of their own at the end): a run of equal scores is three long, and
    # 16 is no multiple of three
    rng = np.random.default_rng(8)
    Q, N = 33, 4097
    codes = np.tile(rng.integers(0, 256, (1365, 256), dtype=np.uint8), (4, 1))[:N]
    scales = np.tile(rng.integers(124, 131, (1365, 16), dtype=np.uint8), (4, 1))[:N]
    codes[4095:] = rng.integers(0, 256, (2, 256), dtype=np.uint8)
    q_int, q_exp = rng.integers(-3, 6, (Q, 512)), rng.integers(-2, 3, Q)
    want, worst = ref.score_c_exact(q_int, np.ldexp(1.0, q_exp), codes, scales)
    assert worst < 2 ** 24
    args = (*_e4m3_rows(q_int, q_exp), _dev(codes), _dev(scales))
    s32, r32 = ops.rank_topk_mxfp4(*args, 32)
    _assert_lists((s32, r32), want, 32)
    s16, r16 = ops.rank_topk_mxfp4(*args, 16)
    below = (s16[:, -1].contiguous(), r16[:, -1].contiguous())
    s2, r2 = ops.rank_topk_mxfp4(*args, 16, below=below)
    assert torch.equal(torch.cat((r16, r2), 1), r32) and torch.equal(torch.cat((s16, s2), 1).view(torch.int32), s32.view(torch.int32))
    dup = (s32[:, 15] == s32[:, 16]).sum().item()                                  # equal scores straddle the cut
    assert dup > 0
    _assert_lists((s2, r2), want, 16, tuple(t.cpu().numpy() for t in below))
    for row in (-1, INT_MAX):
        b = (below[0], torch.full_like(below[1], row))
        _assert_lists(ops.rank_topk_mxfp4(*args, 16, below=b), want, 16, (b[0].cpu().numpy(), b[1].cpu().numpy()))
    # a cutoff below every score: only empty slots
    low = (torch.full_like(below[0], -1e30), torch.full_like(below[1], INT_MAX))
    s0, r0 = ops.rank_topk_mxfp4(*args, 4, below=low)
    assert bool((r0 == INT_MAX).all()) and bool(torch.isinf(s0).all())


def test_the_lists_do_not_depend_on_splits():
    ops = _ops()
    args, want = _exact_case(33, 200003)
    got = [ops.rank_topk_mxfp4(*args, 32, splits=sp) for sp in (1, 7, 256)]
    _assert_lists(got[0], want, 32)
    for g in got[1:]:
        assert torch.equal(g[1], got[0][1]) and torch.equal(g[0].view(torch.int32), got[0][0].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 4. random unit rows
def _unit(n, seed, dev="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, 512, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(dev).contiguous()


def test_sweep_on_unit_rows_against_fp64_and_the_format_error(capsys):
    ops = _ops()
    Q, N, k = 64, 4097, 32
    v, q = _unit(N, 11), _unit(Q, 12)
    codes, scales = ops.quantize_rows_mxfp4(v)
    tq, q_scale = ops.quantize_rows_e4m3(q)
    top_s, top_r = (t.cpu().numpy() for t in ops.rank_topk_mxfp4(tq, q_scale, codes, scales, k))
    a = ref.e4m3_values(tq.cpu().numpy()) * q_scale.cpu().numpy().astype(np.float64)[:, None]
    b = ref.dequantize(codes.cpu().numpy(), scales.cpu().numpy())
    want = a @ b.T
    eps = ACC_EPS * (np.abs(a) @ np.abs(b).T)
    rows = top_r.astype(np.int64)
    err = np.abs(top_s.astype(np.float64) - np.take_along_axis(want, rows, 1))
    ratio = float((err / np.take_along_axis(eps, rows, 1)).max())
    exact = v.double().cpu().numpy() @ q.double().cpu().numpy().T
    fe = (want - exact.T)
    with capsys.disabled():
        print(f"\n[coarse] accumulation: worst |got - fp64| / bound = {ratio:.4f}; format error vs unquantised: rms {np.sqrt((fe ** 2).mean()):.3e}, "
              f"max {np.abs(fe).max():.3e} (Q {Q}, N {N})")
    assert ratio <= 1.0
    assert bool((np.diff(top_s.astype(np.float64), axis=1) <= 0).all())
    # no row outside the list beats the list's last entry by more than the two bounds
    kth = top_s[:, -1].astype(np.float64)[:, None]
    outside = np.ones_like(want, dtype=bool)
    np.put_along_axis(outside, rows, False, 1)
    assert bool((np.where(outside, want, -np.inf) <= kth + 2 * eps.max(1, keepdims=True)).all())


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
class _Identity:
    """A model whose text feature is the embedding itself"""
    @staticmethod
    def get_textual_feature(x):
        return x


VLENS = (7, 300, 64, 65, 1, 500, 263, 130, 170)            # 1500 rows; shards cut after videos 3 and 6
CUTS = (0, 4, 6, 9)
Q_E2E, K_E2E = 5, 10


@functools.lru_cache(maxsize=None)
def _corpus():
    """(rows f32 [N, 512] unit, queries f32 [Q, 512] unit): per query K_E2E rows planted at cosine 0.3 .. 0.6 among random unit rows"""
    N = sum(VLENS)
    v, q = _unit(N, 21, "cpu"), _unit(Q_E2E, 22, "cpu")
    g = torch.Generator().manual_seed(23)
    at = torch.randperm(N, generator=g)[:Q_E2E * K_E2E].reshape(Q_E2E, K_E2E)
    for i in range(Q_E2E):
        for j in range(K_E2E):
            c = 0.3 + 0.3 * j / (K_E2E - 1)
            noise = v[at[i, j]] - (v[at[i, j]] @ q[i]) * q[i]
            v[at[i, j]] = c * q[i] + (1 - c * c) ** 0.5 * noise / noise.norm()
    return v.cuda().contiguous(), q.cuda().contiguous()


def _parts(fmt):
    srch = _srch()
    v, _ = _corpus()
    off = np.concatenate([[0], np.cumsum(VLENS)])
    parts = []
    for a, b in zip(CUTS, CUTS[1:]):
        feat = v[off[a]:off[b]].to(torch.bfloat16 if fmt == "bf16" else torch.float32).contiguous()
        ix = srch.VideoIndex(feat, off[a:b + 1] - off[a], [f"v{j}" for j in range(a, b)])
        parts.append(ix.quantize() if fmt == "e4m3" else ix)
    return parts


def _index(kind, fmt):
    srch = _srch()
    parts = _parts(fmt)
    if kind == "single":
        return srch.VideoIndex.concat(parts)
    if kind == "device":
        return srch.ShardedIndex(parts)
    pinned = [srch.VideoIndex(p.feat.cpu().pin_memory(), p.v_off, p.vids, None if p.scale is None else p.scale.cpu().pin_memory())
              for p in parts]
    return srch.ShardedIndex(pinned, resident="host")


def _embed(strs):
    return _corpus()[1][[int(s) for s in strs]]


def _global_rows(index, hits):
    vnum = {v: i for i, v in enumerate(index.vids)}
    return np.array([[index.v_off[vnum[vid]] + sec for vid, sec, _ in h] for h in hits], dtype=np.int64)


def _bits(hits):
    return [[(vid, sec, np.float32(s).view(np.int32).item()) for vid, sec, s in h] for h in hits]


def _as_stored(x, fmt):
    """f32 rows (device or host) as an index of this row format holds them, f64 on the host"""
    x = x.detach().float().cpu()
    if fmt == "bf16":
        return x.to(torch.bfloat16).double().numpy()
    if fmt == "e4m3":
        codes, scale = _host_e4m3(x)
        return ref.e4m3_values(codes) * scale.astype(np.float64)[:, None]
    return x.double().numpy()


def _precondition(v, q, fmt, k, pool):
    """On the host alone, before the device is asked: every query's exact top k (the fp64 product of the rows as the index stores
    them; the planted rows lead by far more than any f32 sweep's error) lies inside the reference's coarse top `pool`, with a gap to
    entry pool + 1 larger than twice the accumulation bound.  Returns the exact top k rows [Q, k]."""
    rows = _as_stored(v, fmt)
    exact = _as_stored(q, fmt) @ rows.T
    top = np.argsort(-exact, 1, kind="stable")[:, :k]
    assert (np.take_along_axis(exact, top, 1)[:, -1] - np.sort(exact, 1)[:, -k - 1] > 0.05).all()     # the top k is not a near-tie
    codes, scales = ref.quantize(rows.astype(np.float32))
    qc, qs = _host_e4m3(q)
    a = ref.e4m3_values(qc) * qs.astype(np.float64)[:, None]
    b = ref.dequantize(codes, scales)
    sc = a @ b.T
    eps = ACC_EPS * (np.abs(a) @ np.abs(b).T).max(1)
    order = np.sort(sc, 1)[:, ::-1]
    for i in range(sc.shape[0]):
        assert sc[i, top[i]].min() - order[i, pool] > 2 * eps[i], i
    return top


@pytest.mark.parametrize("kind,fmt,pool", [("single", "f32", 32), ("single", "bf16", 32), ("single", "e4m3", 32), ("device", "bf16", 32),
                                           ("host", "bf16", 32), ("host", "e4m3", 70), ("device", "f32", 70)])
def test_search_with_a_coarse_image_equals_the_plain_search(kind, fmt, pool):
    srch = _srch()
    queries = [str(q) for q in range(Q_E2E)]
    top = _precondition(*_corpus(), fmt, K_E2E, pool)
    builder = _index("single" if kind == "single" else "device", fmt)
    image = srch.CoarseImage.build(builder)
    index = _index(kind, fmt)
    plain = srch.search(builder, _Identity, _embed, queries, k=K_E2E)
    assert np.array_equal(np.sort(_global_rows(builder, plain), 1), np.sort(top, 1))
    got = srch.search(index, _Identity, _embed, queries, k=K_E2E, coarse=image, pool=pool)
    assert _bits(got) == _bits(plain)
    assert image.stats["rounds"] == -(-pool // 32) and Q_E2E * K_E2E <= image.stats["unique"] <= Q_E2E * pool
    if kind == "host":
        row_bytes = 516 if fmt == "e4m3" else 1024
        assert index._slots is None                                                # no shard went through the device slots
        assert image.stats["staged_bytes"] == image.stats["unique"] * row_bytes < min(len(p) for p in index.shards) * row_bytes
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ("single", "device", "host"))
def test_a_pool_smaller_than_k_keeps_the_plain_scores_and_order(kind):
    """30 rows in three shards, every row planted near one of three queries: pool = 4 < k = 10 leaves most of a query's top 10
    out of the candidates.  The plain call with k = 30 lists every row: the coarse call's entries are a subsequence of it."""
    srch = _srch()
    q = _unit(3, 32, "cpu")
    v = _unit(30, 33, "cpu")
    for n in range(30):
        c = 0.3 + 0.02 * (n // 3)
        noise = v[n] - (v[n] @ q[n % 3]) * q[n % 3]
        v[n] = c * q[n % 3] + (1 - c * c) ** 0.5 * noise / noise.norm()
    v, q = v.to(torch.bfloat16), q.cuda()
    mk = lambda s, feat: srch.VideoIndex(feat, [0, 4, 10], [f"s{s}a", f"s{s}b"])                                       # noqa: E731
    if kind == "host":
        index = srch.ShardedIndex([mk(s, v[10 * s:10 * s + 10].contiguous().pin_memory()) for s in range(3)], resident="host")
        builder = srch.ShardedIndex([mk(s, v[10 * s:10 * s + 10].cuda().contiguous()) for s in range(3)])
    else:
        builder = srch.ShardedIndex([mk(s, v[10 * s:10 * s + 10].cuda().contiguous()) for s in range(3)])
        if kind == "single":
            builder = srch.VideoIndex.concat(builder.shards)
        index = builder
    image = srch.CoarseImage.build(builder)
    embed = lambda strs: q[[int(s) for s in strs]]                                                                        # noqa: E731
    queries = ["0", "1", "2"]
    full = _bits(srch.search(builder, _Identity, embed, queries, k=30))
    got = _bits(srch.search(index, _Identity, embed, queries, k=10, coarse=image, pool=4))
    assert 4 <= image.stats["unique"] <= 12
    for have, everything in zip(got, full):
        assert len(have) == min(10, image.stats["unique"])
        it = iter(everything)
        assert all(entry in it for entry in have)                                  # a subsequence: same scores, same relative order


def test_shards_smaller_than_a_round_feed_shorter_lists_into_the_fold():
    """Shards of 3 and 2 rows beside one of 200: a round of 32 gets lists of 3 and 2 entries from them (k is clamped to the shard's
    rows), and the cutoff of the second round falls into the large shard.  pool = 40: two rounds."""
    srch = _srch()
    sizes, Q, k, pool = (3, 200, 2), 2, 5, 40
    v, q = _unit(sum(sizes), 41, "cpu"), _unit(Q, 42, "cpu")
    planted = [[0, 2, 100, 203, 204], [1, 3, 50, 150, 203]]                          # rows of all three shards; 203 serves both queries
    for i, rows in enumerate(planted):
        for j, n in enumerate(rows):
            other = q[1 - i] if n == 203 else None
            c = 0.5 + 0.04 * j
            base = c * q[i] + (0.5 * other if other is not None else 0)
            noise = v[n] - (v[n] @ q[0]) * q[0]
            noise = noise - (noise @ q[1]) * q[1]
            v[n] = base + 0.6 * noise / noise.norm()
            v[n] = v[n] / v[n].norm()
    top = _precondition(v, q, "bf16", k, pool)
    v16, off = v.to(torch.bfloat16).cuda(), np.concatenate([[0], np.cumsum(sizes)])
    index = srch.ShardedIndex([srch.VideoIndex(v16[a:b].contiguous(), [0, b - a], [f"s{s}"]) for s, (a, b) in enumerate(zip(off, off[1:]))])
    image = srch.CoarseImage.build(index)
    qd = q.cuda()
    embed = lambda strs: qd[[int(s) for s in strs]]                                                                       # noqa: E731
    plain = srch.search(index, _Identity, embed, ["0", "1"], k=k)
    assert np.array_equal(np.sort(_global_rows(index, plain), 1), np.sort(top, 1))
    got = srch.search(index, _Identity, embed, ["0", "1"], k=k, coarse=image, pool=pool)
    assert _bits(got) == _bits(plain) and image.stats["rounds"] == 2
