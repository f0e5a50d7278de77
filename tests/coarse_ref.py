"""A numpy restatement of the coarse (MXFP4) row format and sweep of include/tan_hip.h, written from the header's words.

Nothing here looks at the kernels: the quantiser goes through frexp and a nearest-value search with ties to the even code, the
scores through fp64 (or exact int64 for integer data), the lists through a plain lexicographic sort."""
import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
EMPTY_ROW = 0x7FFFFFFF


def block_scale_exp(amax):
    """s of a block with this amax (f64 array, finite, >= 0): e - 3 if m <= 0.75 else e - 2, clamped to [-127, 127]; 0 for amax == 0"""
    m, e = np.frexp(np.asarray(amax, dtype=np.float64))
    s = np.where(m <= 0.75, e - 3, e - 2)
    s = np.clip(s, -127, 127)
    return np.where(np.asarray(amax) == 0, 0, s).astype(np.int64)


def rne_e2m1(a):
    """codes 0..7 of magnitudes a (f64, 0 <= a <= 6): the nearest of E2M1, a tie to the even code"""
    a = np.asarray(a, dtype=np.float64)
    d = np.abs(a[..., None] - E2M1)
    best = d.min(-1, keepdims=True)
    near = d == best                                   # one or two neighbouring codes
    even = (np.arange(8) % 2 == 0)
    pick_even = near & even
    code = np.where(near.sum(-1) == 2, pick_even.argmax(-1), near.argmax(-1))
    return code.astype(np.uint8)


def scaled_blocks(x):
    """(x * 2^-s as f64 [n, 16, 32], s int64 [n, 16]) for rows x [n, 512]"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 16, 32)
    s = block_scale_exp(np.abs(x).max(-1))
    return np.ldexp(x, -s[..., None]), s


def quantize(x):
    """rows x [n, 512] (f32, or bf16 values held in f32) -> (codes uint8 [n, 256], scales uint8 [n, 16])"""
    x = np.asarray(x)
    y, s = scaled_blocks(x)
    assert np.abs(y).max(initial=0.0) <= 6.0
    code = rne_e2m1(np.abs(y)) | (np.signbit(np.asarray(x, dtype=np.float64).reshape(y.shape)).astype(np.uint8) << 3)
    code = code.reshape(-1, 256, 2)
    return (code[..., 0] | (code[..., 1] << 4)).astype(np.uint8), (s + 127).astype(np.uint8)


def unpack(codes):
    """codes uint8 [n, 256] -> the elements' unscaled e2m1 values, f64 [n, 512]: element 2 j is byte j's low nibble"""
    codes = np.asarray(codes, dtype=np.uint8)
    nib = np.stack((codes & 15, codes >> 4), -1).reshape(codes.shape[0], 512)
    return np.where(nib & 8, -1.0, 1.0) * E2M1[nib & 7]


def dequantize(codes, scales):
    """(codes, scales) -> f64 [n, 512]"""
    v = unpack(codes).reshape(-1, 16, 32)
    return np.ldexp(v, np.asarray(scales, dtype=np.int64)[..., None] - 127).reshape(-1, 512)


def e4m3_values(codes):
    """OCP e4m3fn bit patterns (uint8) -> f64"""
    c = np.asarray(codes, dtype=np.int64)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, np.ldexp(m / 8.0, -6), np.ldexp(1.0 + m / 8.0, e - 7))
    v = np.where((c & 127) == 127, np.nan, v)
    return np.where(c & 128, -v, v)


def score_c(q_codes, q_scale, codes, scales):
    """score_c [Q, N] in fp64: (sum over blocks of 2^s * sum over the block of qcode * vcode) * q_scale"""
    return (e4m3_values(q_codes) @ dequantize(codes, scales).T) * np.asarray(q_scale, dtype=np.float64)[:, None]


def score_c_exact(q_int, q_scale, codes, scales):
    """For integer query values q_int int64 [Q, 512]: (score_c [Q, N] as exact f64, worst: the largest sum over i of |q_i v_i 2^s| / g
    over all (q, n), g: the power of two every term is a multiple of).  With worst < 2^24 every partial sum in any order is exact
    in f32, and so is the product with the power of two q_scale."""
    s = np.asarray(scales, dtype=np.int64) - 127
    smin = int(s.min())
    v2 = np.rint(unpack(codes) * 2).astype(np.int64).reshape(-1, 16, 32)          # halves
    w = (v2 << (s - smin)[..., None]).reshape(-1, 512)                            # units of g = 2^(smin - 1)
    q_int = np.asarray(q_int, dtype=np.int64)
    assert np.abs(w).max(initial=0) < 2 ** 30
    qf, wf = q_int.astype(np.float64), w.astype(np.float64)                       # integers: fp64 products and sums below 2^53 are exact
    worst = int((np.abs(qf) @ np.abs(wf).T).max())
    assert worst < 2 ** 53
    total = qf @ wf.T
    return np.ldexp(total, smin - 1) * np.asarray(q_scale, dtype=np.float64)[:, None], worst


def after(score, row, below):
    """which (score, row) entries come strictly after the entry `below` = (score, row) in the order score descending, row ascending"""
    bs, br = below
    return (score < bs) | ((score == bs) & (row > br))


def top_list(scores, k, below=None):
    """scores [N] -> (score f32 [k], row int32 [k]): the k best by (score descending, row ascending) of the rows strictly after
    `below`; empty slots are (-inf, EMPTY_ROW)"""
    scores = np.asarray(scores)
    rows = np.arange(scores.shape[0])
    if below is not None:
        rows = rows[after(scores, rows, below)]
    order = rows[np.lexsort((rows, -scores[rows].astype(np.float64)))][:k]
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_r = np.full(k, EMPTY_ROW, dtype=np.int32)
    out_s[:len(order)] = scores[order]
    out_r[:len(order)] = order
    return out_s, out_r


def top_lists(scores, k, below=None):
    """`top_list` per row of scores [Q, N]; below = (score [Q], row [Q])"""
    pairs = [top_list(scores[q], k, None if below is None else (below[0][q], below[1][q])) for q in range(scores.shape[0])]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def shard_cutoff_row(cut_shard, cut_row, s):
    """The cutoff row shard s sweeps with when the cutoff entry lies in shard cut_shard at row cut_row -- the fold's order is (score,
    shard, row): a shard before the cutoff's admits no row at an equal score, a shard after it every one"""
    cut_shard, cut_row = np.asarray(cut_shard), np.asarray(cut_row)
    return np.where(cut_shard == s, cut_row, np.where(s < cut_shard, EMPTY_ROW, -1)).astype(np.int32)


def fold(lists, k):
    """per-shard lists [(score [k_s], row [k_s])] in shard order -> the k best (score, shard, row) by (score desc, shard, row)"""
    sc = np.concatenate([l[0] for l in lists]).astype(np.float64)
    sh = np.concatenate([np.full(len(l[0]), s) for s, l in enumerate(lists)])
    ro = np.concatenate([l[1] for l in lists]).astype(np.int64)
    keep = ro != EMPTY_ROW
    sc, sh, ro = sc[keep], sh[keep], ro[keep]
    order = np.lexsort((ro, sh, -sc))[:k]
    return sc[order].astype(np.float32), sh[order], ro[order]
