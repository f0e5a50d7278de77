"""A numpy statement of `tan_topk_fold` (include/tan_hip.h) and of what folding every shard must give, plus the list makers the
CPU and GPU tests share.  A list is (score [Q, n] f32, shard [Q, n] int32, row [Q, n] int32, aux [n_aux, Q, n] int32)."""
import numpy as np

SENT = 0x7fffffff
SCORES = np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32)           # four values: ties dominate


def empty(Q, k, n_aux):
    return (np.full((Q, k), -np.inf, np.float32), np.full((Q, k), SENT, np.int32), np.full((Q, k), SENT, np.int32),
            np.full((n_aux, Q, k), -1, np.int32))


def _best(score, shard, row, aux, k):
    """The first k of every query's entries under (score descending, shard ascending, row ascending): a stable lexsort."""
    order = np.lexsort((row, shard, -score), axis=-1)[:, :k]
    take = lambda a: np.take_along_axis(a, order, axis=-1)                        # noqa: E731
    return take(score), take(shard), take(row), np.stack([take(a) for a in aux]) if len(aux) else aux[:, :, :k]


def as_entries(incoming, shard):
    """(score [Q, k_in], row [Q, k_in], aux [n_aux, Q, k_in]) of shard `shard` -> a list; slots with row SENT become empty slots"""
    score, row, aux = incoming
    gone = row == SENT
    return (np.where(gone, -np.inf, score).astype(np.float32), np.where(gone, SENT, shard).astype(np.int32), row.astype(np.int32),
            np.where(gone[None], -1, aux).astype(np.int32))


def fold(run, incoming, shard, reset=False):
    """One `tan_topk_fold`: the k best of (run list U incoming list)."""
    k = run[0].shape[1]
    if reset:
        run = empty(run[0].shape[0], k, run[3].shape[0])
    inc = as_entries(incoming, shard)
    return _best(*(np.concatenate((a, b), axis=-1) for a, b in zip(run, inc)), k)


def best_of_all(lists, k):
    """What folding `lists` = {shard: incoming} in ANY order must give: the first k of all their entries, empty slots behind."""
    parts = [as_entries(inc, s) for s, inc in sorted(lists.items())]
    Q, n_aux = parts[0][0].shape[0], parts[0][3].shape[0]
    parts.append(empty(Q, k, n_aux))
    return _best(*(np.concatenate([p[i] for p in parts], axis=-1) for i in range(4)), k)


def aux_of(shard, row, c):
    """The payload a test gives entry (shard, row) in column c: a payload that leaves its key is seen"""
    return ((shard * 1000003 + row * 7 + c * 101) % 2000000011).astype(np.int32)


def make_lists(Q, k_in, n_aux, shards, seed, all_equal=False, sentinels=False, n_rows=50):
    """{shard: (score, row, aux)}: per query k_in DISTINCT rows below n_rows in random order (a fold does not need sorted input),
    scores from SCORES (or all 0.5), payload aux_of.  sentinels: about a third of the slots hold row SENT and a stray score."""
    rng = np.random.default_rng(seed)
    out = {}
    for s in shards:
        row = np.stack([rng.permutation(max(n_rows, k_in))[:k_in] for _ in range(Q)]).astype(np.int32)
        score = np.full((Q, k_in), 0.5, np.float32) if all_equal else SCORES[rng.integers(0, 4, (Q, k_in))]
        if sentinels:
            gone = rng.random((Q, k_in)) < 0.34
            row = np.where(gone, SENT, row).astype(np.int32)
            score = np.where(gone, np.float32(7.0), score).astype(np.float32)
        aux = np.stack([aux_of(np.int64(s), row.astype(np.int64), c) for c in range(n_aux)]) if n_aux else np.zeros((0, Q, k_in), np.int32)
        out[s] = (score, row, aux)
    return out


def same(a, b):
    """bit for bit: scores by their bit patterns"""
    return (np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and np.array_equal(a[3], b[3]))
