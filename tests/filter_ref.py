"""numpy statement of filtered search (include/tan_hip.h "filtered search", `search.RowFilter`), written from the definitions and
independent of search.py: the admitted rows as one boolean per row, the spans read off it, the filter image's tile list and masks,
and the gather-then-map-back oracle (a filtered sweep == the plain sweep over the gathered admitted rows, rows and videos mapped back)."""
import numpy as np

SENT = 0x7FFFFFFF
HEAD = 4                                   # int32 words before the image's tile list


def _numbers(vids, name):
    """the videos `name` means: every video that carries the string, or the video number"""
    if isinstance(name, str):
        found = [v for v, s in enumerate(vids) if s == name]
        if not found:
            raise KeyError(name)
        return found
    if not 0 <= int(name) < len(vids):
        raise KeyError(name)
    return [int(name)]


def admitted_mask(v_off, vids, videos=None, exclude=None, windows=None):
    """bool [N]: row by row.  A video is in when `videos` names it (or is None) and `exclude` does not; an in video that `windows`
    names keeps only the seconds of its windows (inclusive, clamped to the video), any other in video keeps all of its seconds."""
    v_off = np.asarray(v_off, dtype=np.int64)
    nv = len(v_off) - 1
    inside = np.ones(nv, bool) if videos is None else np.zeros(nv, bool)
    for name in (videos or ()):
        inside[_numbers(vids, name)] = True
    for name in (exclude or ()):
        inside[_numbers(vids, name)] = False
    windowed = np.zeros(nv, bool)
    keep = np.zeros(int(v_off[-1]), bool)
    for name, first, last in (windows or ()):
        for v in _numbers(vids, name):
            windowed[v] = True
            vlen = int(v_off[v + 1] - v_off[v])
            for sec in range(max(int(first), 0), min(int(last), vlen - 1) + 1):
                keep[v_off[v] + sec] = True
    mask = np.zeros(int(v_off[-1]), bool)
    for v in range(nv):
        if inside[v]:
            mask[v_off[v]:v_off[v + 1]] = keep[v_off[v]:v_off[v + 1]] if windowed[v] else True
    return mask


def spans_of(mask):
    """int64 [n, 2]: the maximal runs [lo, hi) of True"""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    edges = np.flatnonzero(m[1:] != m[:-1])
    return edges.reshape(-1, 2).astype(np.int64)


def mask_of(spans, N):
    mask = np.zeros(N, bool)
    for lo, hi in np.asarray(spans).reshape(-1, 2):
        mask[lo:hi] = True
    return mask


def videos_with_a_row(mask, v_off):
    return [v for v in range(len(v_off) - 1) if mask[v_off[v]:v_off[v + 1]].any()]


def tile_image(spans, N):
    """(tiles int32 [n_listed] ascending, masks uint64 [n_listed]): the 64-row tiles that hold an admitted row; bit r = row 64 t + r"""
    mask = mask_of(spans, N)
    T = (N + 63) // 64
    padded = np.zeros(T * 64, bool)
    padded[:N] = mask
    bits = (padded.reshape(T, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)[None]).sum(1, dtype=np.uint64)
    tiles = np.flatnonzero(bits != 0).astype(np.int32)
    return tiles, bits[tiles]


def parse_image(img, N):
    """The documented part of a filter image (uint8 numpy of tan_row_filter_bytes(N) bytes) -> (n_listed, T, tiles, masks)"""
    T = (N + 63) // 64
    T2 = (T + 1) // 2 * 2
    words = np.ascontiguousarray(img).view(np.int32)
    n, t_written = int(words[0]), int(words[1])
    assert words[2] == 0 and words[3] == 0
    tiles = words[HEAD:HEAD + n].copy()
    masks = np.ascontiguousarray(img)[4 * (HEAD + T2):4 * (HEAD + T2) + 8 * n].view(np.uint64).copy()
    return n, t_written, tiles, masks


def image_bytes(N):
    T = (N + 63) // 64
    return (4 * (HEAD + (T + 1) // 2 * 2 + 4 * T + (T + 255) // 256) + 15) // 16 * 16


def admitted_rows(spans):
    """int64: the admitted rows in order -- gathered row j of the oracle's index is row admitted_rows[j] of the full one"""
    spans = np.asarray(spans).reshape(-1, 2)
    return np.concatenate([np.arange(lo, hi) for lo, hi in spans] or [np.zeros(0, np.int64)]).astype(np.int64)


def gathered_videos(rows, v_off):
    """(v_off of the gathered index, int64; kept: the full index's video number of every gathered video) -- a video without an
    admitted row is not in the gathered index"""
    v_off = np.asarray(v_off, dtype=np.int64)
    vid = np.searchsorted(v_off, rows, side="right") - 1
    kept, counts = np.unique(vid, return_counts=True)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), kept.astype(np.int64)


def map_back(top_row, rows, fill=SENT):
    """rows of the gathered index -> rows of the full one; a sentinel stays one"""
    top_row = np.asarray(top_row, dtype=np.int64)
    return np.where(top_row == SENT, fill, rows[np.minimum(top_row, len(rows) - 1)])
