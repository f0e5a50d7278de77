"""Corpus sweep time: `ops.rank_topk` over a bf16 index against `ops.rank_topk_e4m3` over the e4m3 index of the same rows, one
process, device events around each call, caller-owned outputs and scratch.  Prints one JSON line; `--out` also writes the table.

    python tools/search_bench.py [--rows 4194304] [--queries 1 64 1024] [-k 10] [--reps 10] [--warmup 3] [--out FILE] [--moments]
    python tools/search_bench.py --sequences [--rows 4194304] [-k 10] [--reps 10] [--warmup 3] [--out FILE]
    python tools/search_bench.py --rerank [--rows 4194304] [--queries 1 64] [--pool 32] [--reps 10] [--warmup 3] [--out FILE]
    python tools/search_bench.py --clips [--rows 4194304] [-k 10] [--reps 10] [--warmup 3] [--out FILE]
    python tools/search_bench.py --copies [--parent-lib PARENT.so] [--rows 4194304] [-k 10] [--reps 10] [--warmup 3] [--out FILE] [--paths-out FILE]
    python tools/search_bench.py --shards [8] [--rows 4194304] [--queries 1 64 1024] [-k 10] [--reps 10] [--warmup 3] [--out FILE]
    python tools/search_bench.py --restrict [--parent-lib PARENT.so] [--rows 4194304] [--queries 1 64 1024] [-k 10] [--out FILE]
    python tools/search_bench.py --annotate [--parent-lib PARENT.so] --rows 1048576 [--labels 128 1024 8192] [--out FILE]

Rows: seeded random unit rows, made in slices.  4 Mi rows are 4 GiB of bf16 and 2 GiB + 16 MiB of e4m3 codes and scales: both far
beyond the 256 MB last-level cache, so every sweep streams its index from HBM.  Bytes per second count the index once per sweep
(at Q <= 128, one query tile, that is all a sweep reads); `of_stream` relates them to the 6.29 TB/s streaming read the project has
measured on this part.  The yardstick is the bf16 sweep of the same run.

--moments adds `ops.rank_topk_video` and `ops.moment_extent` (width 0.07) on the same rows and queries, for two `v_off` layouts:
"corpus" (seeded video lengths 60..1200 seconds) and "one" (a single video of all rows, k = 1: every tile refills the candidate
buffers of a video that is already listed).  `*_video_over_rows` is the video sweep's time over `rank_topk`'s in the same run -- the
same loads and MFMA loop, so the ratio is what the video epilogue and the row -> video map cost.

--sequences times `ops.sequence_topk` INSTEAD of the tables above, on the "corpus" layout, for n_seq x m in 1 x 8, 1 x 32, 8 x 32 and
32 x 32 (random unit steps), bf16 and e4m3.  The yardsticks, in the same run on the same rows with Q = n_seq * m queries, are
`ops.rank_topk_video` (the video sweep) and `ops.rank_topk` (the row sweep).  `finish_ms` is `ops.sequence_scores` plus
`ops.monotonic_decode` for the n_seq * k winners (tables made once, outside the timing).

--clips times `ops.clip_topk` INSTEAD, on the same layout and for the same n_clip x m cases (random unit rows as the clips), bf16 and
e4m3.  The yardsticks, in the same run on the same rows, are `ops.sequence_topk` (the same frame with the scan epilogue) and
`ops.rank_topk` with Q = n_clip * m queries (the row sweep: the same loads and MFMAs); the three alternate call by call.

--copies times `ops.local_align` INSTEAD: P = 32 and 1024 blocks of 128 x 600 and one block of 1200 x 1200 (scores drawn like the
cosines of random unit rows, N(0, 1/512), threshold 0.02, skew 0.01), against two yardsticks in the same run, the three alternating
call by call: `ops.monotonic_decode` over the same blocks (the nearest existing recurrence: global and one-sided) and the host path the
kernel replaces -- read the blocks back and run the float32 anti-diagonal numpy restatement (imported from tests/align_ref.py, the one
file of the test tree this tool depends on: the yardstick is the reference the tests pin, not a second copy of it), timed on the host
clock over the first HOST_BLOCKS blocks and scaled to P where P is larger (`host_scaled`).  `steps` is the kernel's serial chain per
block, ceil(m / 64) * (V + 63) anti-diagonals, and `ns_per_step` the launch's time over it.  Then, on the 4 Mi-row corpus layout over
the bf16 index, `search.search_copies` (a 40-second query cut out of the corpus, pool 32, piece 16, threshold 0.4, skew 0.1) beside
`search.search_clips` (its first 32 seconds), host clock around calls that end in their read-back.  A second table (`paths`,
--paths-out) times `ops.local_align_path` over the same three shapes, alternating call by call with `ops.local_align`:
`path_over_align`, the trace's size and what a caller reads back with and without the map; with --parent-lib the parent commit's
`tan_local_align` runs twice in the same round (`parent_align_ms`, `parent_again_ms`; `parent_spread`: how far its own two medians lie
apart) beside this build's.

--rerank times the stages of `search.search_rerank` INSTEAD, on the "corpus" layout over a bf16 index with a bf16 stem store (random
rows) and a randomly initialised 6 + 6 layer model with the alignability head, bf16: `dual_ms` (`ops.rank_topk_video`, k = pool),
`joint_ms` (per pass of 256 windows: `ops.window_pack` + `joint_from_stem`), `tail_select_ms` (`ops.rerank_tail` per pass +
`ops.rerank_select`), and `end_to_end_ms` (`search_rerank` itself on the host clock: text features, the window table and the read-back
included).  Beside them, same run: `moments_ms` (`rank_topk_video` + `moment_extent` at k = 10: the device work of `search_moments`)
and `eval_windows_ms` (`model.eval_windows` over as many windows of raw 1024-d features: projection, BOTH stacks and the [S, W, T, K]
similarities -- the joint half of it is what stem + tail replace).

--shards [S] times sharded search INSTEAD (`search.ShardedIndex`, S = 8 equal shards of the same rows), bf16 and e4m3, per Q:
`single_ms` (`ops.rank_topk` over the whole index: the yardstick), `device_shards_ms` (S sweeps + S `ops.topk_fold` over device-resident
shards) and their ratio, `fold_us_per_launch` (the S folds alone), `host_shards_ms` (the same loop with the shards streamed from pinned
host memory through `ShardedIndex.shard_views`' two slots) as `host_GBps` of index bytes, and `copy_ms` / `copy_GBps`: a plain pinned
`copy_` of the same bytes into one slot in the same run -- the host link's rate, which `host_shards` cannot beat.  `equals_single`:
the folded lists have the single sweep's scores (bit patterns) and rows.

--restrict times the filtered sweep INSTEAD (`ops.rank_topk_filtered` under `ops.row_filter_build`'s image), bf16 and e4m3, per Q, for
filters that admit 1, 1/2, 1/16 and 1/256 of 64-row videos drawn uniformly with a fixed seed: `build_ms` (the image, apart from the
sweep), `filtered_ms`, `plain_ms` (`ops.rank_topk` over the whole index) beside `parent_plain_ms` (the same entry point of
`--parent-lib`, the parent commit's build, the two alternating call by call in this run), and `gather_ms` (what a caller does without
the feature: `index_select` of the admitted rows, then the plain sweep over them, the gather included).  `equals_gather`: the filtered
lists have the gathered sweep's scores (bit patterns) and rows.

--cover times cover search INSTEAD (`ops.cover_topk`, bf16 and e4m3, one set of m rows for m in --cover-rows; use --rows 1048576):
`cover_topk_ms` beside `label_topk_ms`, `ops.label_topk(k = 1)` at L = m over the same rows -- the same MFMA work in the same
organisation without the two reductions --, the two alternating call by call, and `self_pair_spread`, cover_topk against itself.
--storyboard times storyboards INSTEAD (`search.storyboard`'s two launches over ALL videos of --cover's corpus in one pass, k = 8, bf16 and
e4m3; use --rows 1048576): `scores_ms`, `ops.sequence_scores` with the index's own rows as the queries, and `select_ms`,
`ops.storyboard_select` over its blocks, as `select_GBs` over the k * sum V^2 * 4 bytes it must read (`of_stream`: of STREAM_TBS) -- beside
`torch_ms`, what a caller has without the kernel on the same card from the same blocks: per video k iterations of
`torch.maximum(fix(X), C).sum(1).argmax()` in int64, the two alternating call by call (`equals_torch`: the same seconds, and
the coverage bits that the header's formula makes of the composition's exact int64 sums), `self_pair_spread`, the kernel against itself, and `longest_alone_ms`, the launch over the longest video alone: one workgroup's
serial chain, the tail the launch cannot end before.
--chapters times chapters INSTEAD (`search.chapters`' launches after the scores, over ALL videos of --cover's corpus in one pass, k = 12,
min_len = 5, bf16 and e4m3; use --rows 1048576): `costs_ms` (`ops.chapter_costs`) beside `torch_costs_ms`, and `decode_ms`
(`ops.chapter_decode`) beside `torch_decode_ms` -- what a caller writes without the kernels on the same card from the same blocks: per
video fix(X) in int64, two cumsums, the four-corner difference and `torch.div(..., rounding_mode="floor")`, then per level
`(dp[None, :] + J).min(1)` --, each pair alternating call by call (`same_costs`: the defined triangle bit for bit; `same_scatter`:
every level's dp_j[V] as the header's f32), `*_spread`, each kernel against itself, `costs_GBs` over the 8 bytes per score element the
costs must move (`costs_of_stream`: of STREAM_TBS), `decode_GBs` over the cost elements the levels read, and `longest_*_ms`, the longest
video alone.
--annotate times corpus annotation INSTEAD (`ops.label_topk` / `ops.label_topk_e4m3`, then `ops.label_runs` over its lists), bf16 and
e4m3, for L in --labels and k in --annotate-k (default 1, 5; use --rows 1048576): `label_topk_ms` beside `swapped_rank_ms`, what a caller has without the
entry point -- `ops.rank_topk` with the rows as queries and the labels as the index, over chunks of rows small enough for its scratch
-- the two alternating call by call; `self_pair_spread`, the same alternation of `label_topk` with itself; `torch_ms` (bf16: `matmul`
+ `topk` over the same chunks); `equals_swapped` / `within_eps`: the lists have route (a)'s bits / scores within 2e-5;
`swapped_equals_parent`: this build's `rank_topk` gives what --parent-lib's gives on the first chunk; the achieved FLOP rate and the
label-stream rate it implies; `runs_ms`: `ops.label_runs` at the median best score; `decode_ms`: `ops.label_decode` over the same
lists at that threshold and a penalty of DECODE_SWITCH, timed after `label_topk` in the same run, beside `decode_stream_ms`, the time
its own bytes (N k 8 read, N (k + 1) written and read, N 8 written) would take at HBM_COPY_TBS."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from temporalalignnet_amd import ops  # noqa: E402

STREAM_TBS = 6.29
SLICE = 262144


def unit_rows(n, seed):
    x = torch.randn(n, 512, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")
    return x / x.norm(dim=-1, keepdim=True)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def video_layouts(N):
    lens = np.random.default_rng(0).integers(60, 1201, size=N // 60 + 1)
    cuts = np.concatenate([[0], np.cumsum(lens)])
    corpus = np.concatenate([cuts[cuts < N], [N]])
    return {"corpus": torch.from_numpy(corpus.astype(np.int32)).cuda(), "one": torch.tensor([0, N], dtype=torch.int32, device="cuda")}


def moments_row(Q, N, k, idx, t_rows, a):
    """idx: format -> (tq, vn, scale keywords); t_rows: format -> rank_topk's median ms in this run"""
    row = {}
    for name, v_off in video_layouts(N).items():
        nv = v_off.numel() - 1
        kk = min(k, nv)
        ws = torch.empty(ops.rank_topk_video_ws_bytes(Q, N, nv, kk), dtype=torch.uint8, device="cuda")
        out = (torch.empty(Q, kk, device="cuda"), torch.empty(Q, kk, dtype=torch.int32, device="cuda"),
               torch.empty(Q, kk, dtype=torch.int32, device="cuda"))
        ext = (torch.empty(Q, kk, dtype=torch.int32, device="cuda"), torch.empty(Q, kk, dtype=torch.int32, device="cuda"))
        row[f"{name}_videos"], row[f"{name}_k"] = nv, kk
        for fmt, (tq, vn, kw) in idx.items():
            tv, _ = timed(lambda: ops.rank_topk_video(tq, vn, v_off, kk, out=out, ws=ws, **kw), a.warmup, a.reps)
            te, _ = timed(lambda: ops.moment_extent(tq, vn, v_off, *out, 0.07, out=ext, **kw), a.warmup, a.reps)
            row[f"{name}_{fmt}_video_ms"] = round(tv, 4)
            row[f"{name}_{fmt}_video_over_rows"] = round(tv / t_rows[fmt], 3)
            row[f"{name}_{fmt}_extent_ms"] = round(te, 4)
            row[f"{name}_{fmt}_moment_rows"] = round(float((ext[1] - ext[0] + 1).float().mean()), 1)
    return row


SEQ_CASES = ((1, 8), (1, 32), (8, 32), (32, 32))


def sequences_table(N, k, idx_of, a):
    """idx_of(q f32 [Q, 512]) -> {format: (tq, vn, scale keywords)}"""
    v_off = video_layouts(N)["corpus"]
    v_host = v_off.cpu().numpy().astype(np.int64)
    nv = v_off.numel() - 1
    kk = min(k, nv)
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()          # noqa: E731
    rows = []
    for n_seq, m in SEQ_CASES:
        Q = n_seq * m
        s_off = torch.arange(0, Q + 1, m, dtype=torch.int32, device="cuda")
        for fmt, (tq, vn, kw) in idx_of(unit_rows(Q, (1 << 30) + Q)).items():
            out = (torch.empty(n_seq, kk, device="cuda"), torch.empty(n_seq, kk, dtype=torch.int32, device="cuda"))
            ws = torch.empty(ops.sequence_topk_ws_bytes(n_seq, N, kk), dtype=torch.uint8, device="cuda")
            ts, _ = timed(lambda: ops.sequence_topk(tq, vn, s_off, v_off, kk, out=out, ws=ws, **kw), a.warmup, a.reps)
            vout = (torch.empty(Q, kk, device="cuda"), torch.empty(Q, kk, dtype=torch.int32, device="cuda"),
                    torch.empty(Q, kk, dtype=torch.int32, device="cuda"))
            vws = torch.empty(ops.rank_topk_video_ws_bytes(Q, N, nv, kk), dtype=torch.uint8, device="cuda")
            tv, _ = timed(lambda: ops.rank_topk_video(tq, vn, v_off, kk, out=vout, ws=vws, **kw), a.warmup, a.reps)
            rout = (None, None, vout[0], vout[1])
            rws = torch.empty(ops.rank_topk_ws_bytes(Q, N, kk), dtype=torch.uint8, device="cuda")
            if kw:
                tr, _ = timed(lambda: ops.rank_topk_e4m3(tq, kw["q_scale"], vn, kw["v_scale"], None, kk, out=rout, ws=rws), a.warmup, a.reps)
            else:
                tr, _ = timed(lambda: ops.rank_topk(tq, vn, None, kk, out=rout, ws=rws), a.warmup, a.reps)
            # the winners' seconds: one [m, V] block per hit, then the decode over them
            video = out[1].cpu().numpy().astype(np.int64).reshape(-1)
            P = n_seq * kk
            hv = v_host[video + 1] - v_host[video]
            x_off = np.concatenate([[0], np.cumsum(m * hv)])
            first = np.arange(P + 1) * m
            hit_of_row = np.repeat(np.arange(P), m)
            rows_t = i32(np.stack((x_off[hit_of_row] + (np.arange(P * m) - first[hit_of_row]) * hv[hit_of_row], hv[hit_of_row]), 1))
            vtab = i32(np.stack((first[:-1], np.full(P, m), np.concatenate([[0], np.cumsum(hv)])[:-1]), 1))
            hits = i32(np.stack((np.repeat(np.arange(n_seq), kk), video), 1))
            xo = torch.from_numpy(x_off[:-1].copy()).cuda()
            x = torch.empty(int(x_off[-1]), device="cuda")
            order = torch.arange(P * m, dtype=torch.int32, device="cuda")
            bp, run = torch.empty(x.numel(), dtype=torch.int32, device="cuda"), torch.empty(int(hv.sum()), device="cuda")
            sec, path = torch.empty(P * m, dtype=torch.int32, device="cuda"), torch.empty(P, device="cuda")

            def finish():
                ops.sequence_scores(tq, vn, s_off, v_off, hits, xo, x, **kw)
                ops.monotonic_decode(x, rows_t, order, vtab, None, bp, run, sec, path)
            tf, _ = timed(finish, a.warmup, a.reps)
            rows.append({"n_seq": n_seq, "m": m, "fmt": fmt, "Q": Q, "videos": nv, "k": kk, "sequence_ms": round(ts, 4),
                         "video_sweep_ms": round(tv, 4), "row_sweep_ms": round(tr, 4), "seq_over_video": round(ts / tv, 3),
                         "seq_over_rows": round(ts / tr, 3), "finish_ms": round(tf, 4), "hit_rows": int(hv.sum()),
                         "path_equals_decode": bool(torch.equal(path.view(n_seq, kk), out[0]))})
    return rows


def clips_table(N, k, idx_of, a):
    """idx_of(q f32 [Q, 512]) -> {format: (tq, vn, scale keywords)}"""
    v_off = video_layouts(N)["corpus"]
    nv = v_off.numel() - 1
    kk = min(k, nv)
    rows = []
    for n_clip, m in SEQ_CASES:
        Q = n_clip * m
        c_off = torch.arange(0, Q + 1, m, dtype=torch.int32, device="cuda")
        for fmt, (tq, vn, kw) in idx_of(unit_rows(Q, (1 << 30) + Q)).items():
            out = (torch.empty(n_clip, kk, device="cuda"), torch.empty(n_clip, kk, dtype=torch.int32, device="cuda"),
                   torch.empty(n_clip, kk, dtype=torch.int32, device="cuda"))
            ws = torch.empty(ops.clip_topk_ws_bytes(n_clip, N, kk), dtype=torch.uint8, device="cuda")
            sout = (torch.empty(n_clip, kk, device="cuda"), torch.empty(n_clip, kk, dtype=torch.int32, device="cuda"))
            sws = torch.empty(ops.sequence_topk_ws_bytes(n_clip, N, kk), dtype=torch.uint8, device="cuda")
            rout = (None, None, torch.empty(Q, kk, device="cuda"), torch.empty(Q, kk, dtype=torch.int32, device="cuda"))
            rws = torch.empty(ops.rank_topk_ws_bytes(Q, N, kk), dtype=torch.uint8, device="cuda")

            def rows_sweep():
                if kw:
                    ops.rank_topk_e4m3(tq, kw["q_scale"], vn, kw["v_scale"], None, kk, out=rout, ws=rws)
                else:
                    ops.rank_topk(tq, vn, None, kk, out=rout, ws=rws)
            tc, ts, tr = timed_round((lambda: ops.clip_topk(tq, vn, c_off, v_off, kk, out=out, ws=ws, **kw),
                                      lambda: ops.sequence_topk(tq, vn, c_off, v_off, kk, out=sout, ws=sws, **kw), rows_sweep),
                                     a.warmup, a.reps)
            # a placement is one of the order-preserving paths and a rounded add is monotone: the j-th best match never exceeds the j-th best path
            below = bool((out[0] <= sout[0]).all())
            rows.append({"n_clip": n_clip, "m": m, "fmt": fmt, "Q": Q, "videos": nv, "k": kk, "clip_ms": round(tc, 4),
                         "sequence_ms": round(ts, 4), "row_sweep_ms": round(tr, 4), "clip_over_seq": round(tc / ts, 3),
                         "clip_over_rows": round(tc / tr, 3), "match_le_path": below})
    return rows


ALIGN_CASES = ((32, 128, 600), (1024, 128, 600), (1, 1200, 1200))
ALIGN_PRICES = (0.02, 0.01)
HOST_BLOCKS = 8


def copies_table(N, k, v16, a):
    import time

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import align_ref

    from temporalalignnet_amd import search
    theta, skew = ALIGN_PRICES
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()          # noqa: E731
    rows, paths = [], []
    parent = parent_align(a.parent_lib) if a.parent_lib else None
    for P, m, V in ALIGN_CASES:
        x = torch.randn(P * m * V, generator=torch.Generator(device="cuda").manual_seed(P + m), device="cuda") * (512 ** -0.5)
        x_off = torch.arange(P, dtype=torch.int64, device="cuda") * (m * V)
        table = i32(np.stack((np.full(P, m), np.full(P, V), np.arange(P) * V), 1))
        out = (torch.empty(P, device="cuda"), torch.empty(P, 5, dtype=torch.int32, device="cuda"))
        ws = torch.empty(ops.local_align_ws_bytes(P, P * V), dtype=torch.uint8, device="cuda")
        # the decode's tables: one "video" per block, its m rows in order
        hit_of_row = np.repeat(np.arange(P), m)
        rows_t = i32(np.stack((hit_of_row * m * V + (np.arange(P * m) % m) * V, np.full(P * m, V)), 1))
        vtab = i32(np.stack((np.arange(P) * m, np.full(P, m), np.arange(P) * V), 1))
        order = torch.arange(P * m, dtype=torch.int32, device="cuda")
        bp, run = torch.empty(x.numel(), dtype=torch.int32, device="cuda"), torch.empty(P * V, device="cuda")
        sec, path = torch.empty(P * m, dtype=torch.int32, device="cuda"), torch.empty(P, device="cuda")
        n_host = min(P, HOST_BLOCKS)
        host_ms, host_out = [], []

        def host():
            t0 = time.perf_counter()
            back = x.cpu().numpy()
            t1 = time.perf_counter()
            host_out[:] = [align_ref.align(back[h * m * V:(h + 1) * m * V].reshape(m, V), theta, skew) for h in range(n_host)]
            host_ms.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        ta, td, _ = timed_round((lambda: ops.local_align(x, x_off, table, theta, skew, sum_V=P * V, out=out, ws=ws),
                                 lambda: ops.monotonic_decode(x, rows_t, order, vtab, None, bp, run, sec, path), host), a.warmup, a.reps)
        back_ms, ref_ms = (float(np.median([t[i] for t in host_ms[a.warmup:]])) for i in (0, 1))
        sc, sp = out[0].cpu().numpy(), out[1].cpu().numpy()
        same = all(sc[h:h + 1].view(np.int32)[0] == np.array([w[0]]).view(np.int32)[0] and tuple(sp[h].tolist()) == w[1]
                   for h, w in enumerate(host_out))
        steps = (m + 63) // 64 * (V + 63)
        rows.append({"P": P, "m": m, "V": V, "local_align_ms": round(ta, 4), "monotonic_decode_ms": round(td, 4),
                     "align_over_decode": round(ta / td, 3), "steps": steps, "ns_per_step": round(ta * 1e6 / steps, 1),
                     "Mcells_per_s": round(P * m * V / ta * 1e-3, 1), "read_back_ms": round(back_ms, 3), "host_blocks": n_host,
                     "host_ref_ms": round(ref_ms, 1), "host_scaled_ms": round(back_ms + ref_ms * P / n_host, 1),
                     "host_over_align": round((back_ms + ref_ms * P / n_host) / ta, 1), "equals_host": bool(same)})
        # the same blocks with the time map: local_align and local_align_path alternate call by call; with --parent-lib the parent
        # commit's tan_local_align runs TWICE in the same round, and the distance of its two medians is the session's spread
        path_off, n_map, n_trace = search.path_tables(np.full(P, m), np.full(P, V))
        po = torch.from_numpy(path_off).cuda()
        pout = (torch.empty(P, device="cuda"), torch.empty(P, 5, dtype=torch.int32, device="cuda"),
                torch.empty(n_map, 2, dtype=torch.int32, device="cuda"))
        pws = torch.empty(ops.local_align_path_ws_bytes(P, P * V, n_trace), dtype=torch.uint8, device="cuda")
        fns = [lambda: ops.local_align(x, x_off, table, theta, skew, sum_V=P * V, out=out, ws=ws),
               lambda: ops.local_align_path(x, x_off, table, theta, skew, po, sum_V=P * V, n_map=n_map, n_trace=n_trace, out=pout, ws=pws)]
        if parent is not None:
            pout0 = (torch.empty(P, device="cuda"), torch.empty(P, 5, dtype=torch.int32, device="cuda"))
            fns += [lambda: parent(x, x_off, table, P, P * V, theta, skew, pout0, ws)] * 2
        t = timed_round(fns, a.warmup, a.reps)
        aligned = pout[1][:, 4] > 0
        lo, hi = pout[2].view(P, m, 2)[..., 0], pout[2].view(P, m, 2)[..., 1]
        prow = {"P": P, "m": m, "V": V, "local_align_ms": round(t[0], 4), "local_align_path_ms": round(t[1], 4),
                "path_over_align": round(t[1] / t[0], 3), "trace_MB": round(16 * n_trace / 1e6, 2), "align_read_back_bytes": 24 * P,
                "path_read_back_bytes": 24 * P + 8 * n_map, "mean_cells": round(float(pout[1][:, 4].float().mean()), 1),
                "same_score_span": bool(torch.equal(pout[0].view(torch.int32), out[0].view(torch.int32)) and torch.equal(pout[1], out[1])),
                "cells_add_up": bool(torch.equal(((hi - lo + 1) * (lo >= 0)).sum(1)[aligned], pout[1][aligned, 4].long()))}
        if parent is not None:
            prow.update({"parent_align_ms": round(t[2], 4), "parent_again_ms": round(t[3], 4),
                         "parent_spread": round(abs(t[2] - t[3]) / min(t[2], t[3]), 4), "align_over_parent": round(t[0] / min(t[2], t[3]), 4),
                         "equals_parent": bool(torch.equal(pout0[0].view(torch.int32), out[0].view(torch.int32)) and torch.equal(pout0[1], out[1]))})
        paths.append(prow)
        del x, bp, pws
    # end to end on the corpus layout: one 40-second query cut out of a video
    v_off = video_layouts(N)["corpus"].cpu().numpy().astype(np.int64)
    idx = search.VideoIndex(v16, v_off, [f"v{i:06d}" for i in range(len(v_off) - 1)])
    src = int(np.argmax(v_off[1:] - v_off[:-1] >= 100))
    query, clip = (src, 30, 69), (src, 30, 61)

    def host_clock(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))
    found = search.search_copies(idx, [query], k=k, threshold=0.4, skew=0.1)[0]
    t_copies = host_clock(lambda: search.search_copies(idx, [query], k=k, threshold=0.4, skew=0.1))
    t_clips = host_clock(lambda: search.search_clips(idx, [clip], k=k))
    e2e = {"videos": len(v_off) - 1, "query_seconds": 40, "pool": 32, "piece": 16, "search_copies_ms": round(t_copies, 3),
           "search_clips_ms": round(t_clips, 3), "copies_over_clips": round(t_copies / t_clips, 3), "hits": len(found),
           "finds_its_source": bool(found and found[0][:5] == (idx.vids[src], 30, 69, 0, 39))}
    t_paths = host_clock(lambda: search.search_copies(idx, [query], k=k, threshold=0.4, skew=0.1, paths=True))
    e2e["search_copies_paths_ms"] = round(t_paths, 3)
    return rows, e2e, paths


def shards_table(N, k, v16, v8, s8, a):
    """One row per (format, Q): the single sweep, S device-resident shards, S host-resident shards, the fold alone, a plain pinned
    copy of the same bytes."""
    from temporalalignnet_amd import search
    S = a.shards
    cuts = [N * i // S for i in range(S + 1)]
    base = torch.tensor(cuts[:-1], device="cuda")
    rows = []
    for fmt, vn, vs, row_bytes in (("bf16", v16, None, 1024), ("e4m3", v8, s8, 516)):
        parts = [search.VideoIndex(vn[c0:c1], [0, c1 - c0], [f"s{i}"], None if vs is None else vs[c0:c1])
                 for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:]))]
        dev = search.ShardedIndex(parts)
        host = search.ShardedIndex([search.VideoIndex(p.feat.cpu().pin_memory(), p.v_off, p.vids, None if vs is None else p.scale.cpu().pin_memory())
                                    for p in parts], resident="host")
        n_max = max(len(p) for p in parts)
        slot = torch.empty(n_max, 512, dtype=vn.dtype, device="cuda")
        slot_s = torch.empty(n_max, device="cuda") if vs is not None else None

        def copy_all():
            for p in host.shards:
                slot[:len(p)].copy_(p.feat, non_blocking=True)
                if vs is not None:
                    slot_s[:len(p)].copy_(p.scale, non_blocking=True)
        t_copy, _ = timed(copy_all, a.warmup, a.reps)
        for Q in a.queries:
            q = unit_rows(Q, 1 << 30)
            tq, qs = (q.to(torch.bfloat16), None) if vs is None else ops.quantize_rows_e4m3(q)
            ws = torch.empty(max(ops.rank_topk_ws_bytes(Q, n, k) for n in [N] + [len(p) for p in parts]), dtype=torch.uint8, device="cuda")
            one = (None, None, torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
            out = (None, None, torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
            run = (torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"),
                   torch.empty(Q, k, dtype=torch.int32, device="cuda"), None)

            def sweep(feat, scale, o):
                if vs is None:
                    ops.rank_topk(tq, feat, None, k, out=o, ws=ws)
                else:
                    ops.rank_topk_e4m3(tq, qs, feat, scale, None, k, out=o, ws=ws)

            def sharded(index):
                for i, (s, feat, scale, _) in enumerate(index.shard_views()):
                    sweep(feat, scale, out)
                    ops.topk_fold(run, out[2:], s, reset=i == 0)

            def folds():
                for s in range(S):
                    ops.topk_fold(run, out[2:], s, reset=s == 0)
            t_one, _ = timed(lambda: sweep(vn, vs, one), a.warmup, a.reps)
            t_dev, _ = timed(lambda: sharded(dev), a.warmup, a.reps)
            same_dev = bool(torch.equal(run[0].view(torch.int32), one[2].view(torch.int32)) and torch.equal(base[run[1].long()] + run[2], one[3].long()))
            t_fold, _ = timed(folds, a.warmup, a.reps)
            t_host, _ = timed(lambda: sharded(host), a.warmup, a.reps)
            same_host = bool(torch.equal(run[0].view(torch.int32), one[2].view(torch.int32)) and torch.equal(base[run[1].long()] + run[2], one[3].long()))
            rows.append({"fmt": fmt, "Q": Q, "shards": S, "single_ms": round(t_one, 4), "device_shards_ms": round(t_dev, 4),
                         "device_over_single": round(t_dev / t_one, 3), "fold_us_per_launch": round(t_fold / S * 1e3, 2),
                         "host_shards_ms": round(t_host, 3), "host_GBps": round(N * row_bytes / t_host * 1e-6, 2),
                         "copy_ms": round(t_copy, 3), "copy_GBps": round(N * row_bytes / t_copy * 1e-6, 2),
                         "host_over_copy": round(t_host / t_copy, 3), "equals_single": same_dev and same_host})
        del host, slot, slot_s
    return rows


RESTRICT_FRACTIONS = ((1, 1), (1, 2), (1, 16), (1, 256))
RESTRICT_VLEN = 64


def timed_pair(fa, fb, warmup, reps):
    """Median ms of fa and of fb, the two alternating call by call (A B A B ...): what one of them gains from the other's leftovers in
    the caches, or loses to a neighbour on the machine, the other gets too."""
    for _ in range(warmup):
        fa()
        fb()
    ms = ([], [])
    for _ in range(reps):
        for fn, acc in ((fa, ms[0]), (fb, ms[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return float(np.median(ms[0])), float(np.median(ms[1]))


def timed_round(fns, warmup, reps):
    """`timed_pair` for any number of routines: their median ms, the routines alternating call by call (A B C A B C ...)"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for fn, acc in zip(fns, ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return [float(np.median(x)) for x in ms]


def parent_sweep(path):
    """The plain sweep entry points of ANOTHER build of the library (the parent commit's), called as `ops.rank_topk` calls them"""
    import ctypes as C

    from temporalalignnet_amd import _lib
    L, protos = C.CDLL(path), _lib.declared_prototypes()
    for name in ("tan_rank_topk", "tan_rank_topk_e4m3"):
        getattr(L, name).restype, getattr(L, name).argtypes = protos[name]

    def run(tq, vn, kw, k, out, ws):
        Q, N, st = tq.shape[0], vn.shape[0], torch.cuda.current_stream().cuda_stream
        if kw:
            rc = L.tan_rank_topk_e4m3(tq.data_ptr(), kw["q_scale"].data_ptr(), vn.data_ptr(), kw["v_scale"].data_ptr(), Q, N, 512, None, k, 0,
                                      None, None, out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), st)
        else:
            rc = L.tan_rank_topk(tq.data_ptr(), vn.data_ptr(), ops.TAN_BF16, Q, N, 512, None, k, 0, None, None, out[0].data_ptr(),
                                 out[1].data_ptr(), ws.data_ptr(), st)
        assert rc == 0, rc
    return run


def parent_align(path):
    """tan_local_align of ANOTHER build of the library (the parent commit's), called as `ops.local_align` calls it"""
    import ctypes as C

    from temporalalignnet_amd import _lib
    L = C.CDLL(path)
    L.tan_local_align.restype, L.tan_local_align.argtypes = _lib.declared_prototypes()["tan_local_align"]

    def run(x, x_off, table, P, sum_V, theta, skew, out, ws):
        rc = L.tan_local_align(x.data_ptr(), x.numel(), x_off.data_ptr(), table.data_ptr(), P, sum_V, theta, skew, out[0].data_ptr(),
                               out[1].data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return run


def restrict_table(N, k, v16, v8, s8, a):
    """One row per (format, Q, admitted fraction): whole videos of 64 rows drawn uniformly with a fixed seed.  build_ms =
    `ops.row_filter_build` (spans already on the device); filtered_ms = `ops.rank_topk_filtered`; plain_ms = `ops.rank_topk` over the
    whole index, and parent_plain_ms the same entry point of --parent-lib, the two alternating call by call; gather_ms = what a
    caller does without the feature: `index_select` of the admitted rows (and scales), then `ops.rank_topk` over them."""
    nv = N // RESTRICT_VLEN
    parent = parent_sweep(a.parent_lib) if a.parent_lib else None
    rows = []
    for fmt, vn, vs in (("bf16", v16, None), ("e4m3", v8, s8)):
        for Q in a.queries:
            q = unit_rows(Q, 1 << 30)
            tq, qs = (q.to(torch.bfloat16), None) if vs is None else ops.quantize_rows_e4m3(q)
            kw = {} if vs is None else dict(q_scale=qs, v_scale=vs)
            ws = torch.empty(ops.rank_topk_ws_bytes(Q, N, k), dtype=torch.uint8, device="cuda")
            out = (torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
            pout = (torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))

            def plain(feat=vn, scales=kw, o=out):
                if scales:
                    ops.rank_topk_e4m3(tq, qs, feat, scales["v_scale"], None, k, out=(None, None, *o), ws=ws)
                else:
                    ops.rank_topk(tq, feat, None, k, out=(None, None, *o), ws=ws)
            if parent:
                t_plain, t_parent = timed_pair(plain, lambda: parent(tq, vn, kw, k, pout, ws), a.warmup, a.reps)
                same_parent = bool(torch.equal(out[0].view(torch.int32), pout[0].view(torch.int32)) and torch.equal(out[1], pout[1]))
            else:
                (t_plain, _), t_parent, same_parent = timed(plain, a.warmup, a.reps), None, None
            for num, den in RESTRICT_FRACTIONS:
                picked = np.sort(np.random.default_rng(den).permutation(nv)[:nv * num // den]).astype(np.int64)
                edge = np.flatnonzero(np.diff(picked) != 1)                                    # adjacent videos merge into one span
                first, last = picked[np.concatenate([[0], edge + 1])], picked[np.concatenate([edge, [len(picked) - 1]])]
                spans = torch.from_numpy(np.stack((first, last + 1), 1).astype(np.int32) * RESTRICT_VLEN).cuda()
                rows_t = (torch.from_numpy(picked).cuda()[:, None] * RESTRICT_VLEN + torch.arange(RESTRICT_VLEN, device="cuda")[None]).reshape(-1)
                filt = torch.empty(ops.row_filter_bytes(N), dtype=torch.uint8, device="cuda")
                t_build, _ = timed(lambda: ops.row_filter_build(spans, N, out=filt), a.warmup, a.reps)
                t_filt, _ = timed(lambda: ops.rank_topk_filtered(tq, vn, filt, k, out=out, ws=ws, **kw), a.warmup, a.reps)
                got_s, got_r = out[0].clone(), out[1].clone()

                def gather():
                    g = torch.index_select(vn, 0, rows_t)
                    plain(g, dict(v_scale=torch.index_select(vs, 0, rows_t)) if kw else {}, pout)
                t_gather, _ = timed(gather, a.warmup, a.reps)
                same = bool(torch.equal(got_s.view(torch.int32), pout[0].view(torch.int32)) and torch.equal(got_r.long(), rows_t[pout[1].long()]))
                rows.append({"fmt": fmt, "Q": Q, "fraction": f"{num}/{den}", "spans": int(spans.shape[0]), "admitted_rows": int(rows_t.numel()),
                             "build_ms": round(t_build, 4), "filtered_ms": round(t_filt, 4), "plain_ms": round(t_plain, 4),
                             "parent_plain_ms": None if t_parent is None else round(t_parent, 4),
                             "plain_over_parent": None if t_parent is None else round(t_plain / t_parent, 3),
                             "filtered_over_plain": round(t_filt / t_plain, 4), "filtered_over_fraction": round(t_filt / (t_plain * num / den), 3),
                             "gather_ms": round(t_gather, 4), "gather_over_filtered": round(t_gather / t_filt, 2),
                             "equals_gather": same, "plain_equals_parent": same_parent})
                del rows_t, filt
    return rows


ANNOTATE_KS = (1, 5)
ANNOTATE_CHUNK = 65536            # route (a): rows per roles-swapped rank_topk call; its scratch is (label tiles, at most 256) x chunk x k x 8 bytes
DECODE_SWITCH, HBM_COPY_TBS = 0.02, 6.29   # the decode's penalty per label change; the measured float4 copy rate (MI355X_MICROARCH)
BF16_MFMA_PEAK_TF, L2_SHARED_TBS, INF_CACHE_TBS = 2500.0, (16.8, 18.8), 8.6      # MI355X_MICROARCH figures, not measurements of this kernel


def annotate_table(N, v16, v8, s8, a):
    """One row per (format, L, k): `ops.label_topk` over N rows against L labels, alternating call by call with route (a), what a caller
    has without it: `ops.rank_topk` with the roles swapped (the rows as queries, the labels as the index) over chunks of ANNOTATE_CHUNK
    rows; bf16 also route (b), torch `matmul` + `topk` over the same chunks; then `ops.label_runs` over the result."""
    parent = parent_sweep(a.parent_lib) if a.parent_lib else None
    v_off = video_layouts(N)["corpus"]
    rows = []
    for fmt, vn, vs, row_bytes in (("bf16", v16, None, 1024), ("e4m3", v8, s8, 512)):
        for L in a.labels:
            lab = unit_rows(L, (1 << 29) + L)
            tl, ls = (lab.to(torch.bfloat16), None) if vs is None else ops.quantize_rows_e4m3(lab)
            for k in [k for k in a.annotate_k if k <= L]:
                out = (torch.empty(N, k, device="cuda"), torch.empty(N, k, dtype=torch.int32, device="cuda"))
                ref = (torch.empty(N, k, device="cuda"), torch.empty(N, k, dtype=torch.int32, device="cuda"))
                chunk = min(ANNOTATE_CHUNK, N)
                ws = torch.empty(ops.rank_topk_ws_bytes(chunk, L, k), dtype=torch.uint8, device="cuda")

                def new():
                    if vs is None:
                        ops.label_topk(tl, vn, k, out=out)
                    else:
                        ops.label_topk_e4m3(tl, ls, vn, vs, k, out=out)

                def swapped(o=ref):
                    for c0 in range(0, N, chunk):
                        c1 = min(c0 + chunk, N)
                        if vs is None:
                            ops.rank_topk(vn[c0:c1], tl, None, k, out=(None, None, o[0][c0:c1], o[1][c0:c1]), ws=ws)
                        else:
                            ops.rank_topk_e4m3(vn[c0:c1], vs[c0:c1], tl, ls, None, k, out=(None, None, o[0][c0:c1], o[1][c0:c1]), ws=ws)
                t_new, t_a = timed_pair(new, swapped, a.warmup, a.reps)
                t_new2, t_new3 = timed_pair(new, new, a.warmup, a.reps)                     # the spread of alternating calls of ONE routine
                same = bool(torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(out[1], ref[1]))
                within = bool(((out[0] - ref[0]).abs() <= 2e-5).all())
                same_parent = None
                if parent:                                                                  # this build's unchanged sweep against the parent's, one chunk
                    pout = (torch.empty(chunk, k, device="cuda"), torch.empty(chunk, k, dtype=torch.int32, device="cuda"))
                    kw = {} if vs is None else dict(q_scale=vs[:chunk], v_scale=ls)
                    parent(vn[:chunk], tl, kw, k, pout, ws)
                    same_parent = bool(torch.equal(pout[0].view(torch.int32), ref[0][:chunk].view(torch.int32)) and torch.equal(pout[1], ref[1][:chunk]))
                t_b = None
                if vs is None:
                    def torch_route():
                        for c0 in range(0, N, chunk):
                            s, i = (vn[c0:c0 + chunk] @ tl.T).topk(k, dim=1)
                    t_b, _ = timed(torch_route, a.warmup, a.reps)
                thr = float(out[0][:, 0].median())
                cap = N
                runs = (torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(5, cap, dtype=torch.int32, device="cuda"),
                        torch.empty(cap, device="cuda"), torch.empty(L, dtype=torch.int32, device="cuda"))
                rws = torch.empty(ops.label_runs_ws_bytes(N), dtype=torch.uint8, device="cuda")
                t_runs, _ = timed(lambda: ops.label_runs(out[0], out[1], L, v_off, thr, 1, cap=cap, out=runs, ws=rws), a.warmup, a.reps)
                dec = (torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, device="cuda"))
                dws = torch.empty(ops.label_decode_ws_bytes(N, k), dtype=torch.uint8, device="cuda")
                t_dec, _ = timed(lambda: ops.label_decode(out[0], out[1], v_off, thr, DECODE_SWITCH, out=dec, ws=dws), a.warmup, a.reps)
                dec_bytes = N * k * 8 + 2 * N * (k + 1) + N * 8
                tflops = 2.0 * N * L * 512 / t_new * 1e-9
                stream = -(-N // 128) * L * row_bytes / t_new * 1e-9                         # TB/s: every workgroup of 128 rows reads every label once
                rows.append({"fmt": fmt, "L": L, "k": k, "label_topk_ms": round(t_new, 4), "swapped_rank_ms": round(t_a, 4),
                             "new_over_swapped": round(t_new / t_a, 4), "self_pair_spread": round(abs(t_new2 / t_new3 - 1), 4),
                             "torch_ms": None if t_b is None else round(t_b, 4), "TFLOPs": round(tflops, 1),
                             "of_bf16_mfma_peak": round(tflops / BF16_MFMA_PEAK_TF, 4) if vs is None else None,
                             "label_stream_TBps": round(stream, 2), "equals_swapped": same, "within_eps": within,
                             "swapped_equals_parent": same_parent, "runs_ms": round(t_runs, 4), "runs": int(runs[0][0]),
                             "rows_kept": int(runs[3].sum()), "decode_ms": round(t_dec, 4),
                             "decode_stream_ms": round(dec_bytes / HBM_COPY_TBS * 1e-9, 4), "decoded_rows": int((dec[0] >= 0).sum())})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)                      # progress: a row takes seconds
                del out, ref, ws, runs, rws, dec, dws
    return rows


def cover_table(N, v16, v8, s8, a):
    """One row per (format, m): `ops.cover_topk` of ONE set of m rows over N rows in videos of 60 to 1 200 rows (rank "both", k = 10,
    caller-owned outputs), alternating call by call with `ops.label_topk(k = 1)` at L = m over the same rows -- the same MFMA work in
    the same organisation, without the two reductions -- and `self_pair_spread`, the same alternation of cover_topk with itself."""
    v_off = video_layouts(N)["corpus"]
    nv = v_off.numel() - 1
    rows = []
    for fmt in ("bf16", "e4m3"):
        for m in a.cover_rows:
            q = unit_rows(m, 9000 + m)
            q_off = torch.tensor([0, m], dtype=torch.int32, device="cuda")
            out = (torch.empty(1, 10, device="cuda"), torch.empty(1, 10, dtype=torch.int32, device="cuda"),
                   torch.empty(1, 10, dtype=torch.int32, device="cuda"), torch.empty(1, nv, device="cuda"), torch.empty(1, nv, device="cuda"))
            lab = (torch.empty(N, 1, device="cuda"), torch.empty(N, 1, dtype=torch.int32, device="cuda"))
            if fmt == "bf16":
                tq = q.to(torch.bfloat16)
                cover = lambda: ops.cover_topk(tq, v16, q_off, v_off, 10, out=out)           # noqa: E731
                label = lambda: ops.label_topk(tq, v16, 1, out=lab)                          # noqa: E731
            else:
                tq, qs = ops.quantize_rows_e4m3(q)
                cover = lambda: ops.cover_topk(tq, v8, q_off, v_off, 10, q_scale=qs, v_scale=s8, out=out)   # noqa: E731
                label = lambda: ops.label_topk_e4m3(tq, qs, v8, s8, 1, out=lab)              # noqa: E731
            t_new, t_lab = timed_pair(cover, label, a.warmup, a.reps)
            s_a, s_b = timed_pair(cover, cover, a.warmup, a.reps)
            rows.append({"fmt": fmt, "m": m, "videos": nv, "cover_topk_ms": round(t_new, 4), "label_topk_ms": round(t_lab, 4),
                         "new_over_label": round(t_new / t_lab, 4), "self_pair_spread": round(abs(s_a / s_b - 1), 4),
                         "TFLOPs": round(2 * N * m * 512 / t_new / 1e9, 1)})
    return rows


STORYBOARD_K = 8


def torch_storyboard(x, x_off, lens, k, second, total):
    """What a caller writes without tan_storyboard_select, from the same blocks: per video k iterations of
    `torch.maximum(fix(X), C).sum(1).argmax()` in int64 (k <= every V and no stop test: random rows always gain); no host round trip.
    second int32 [P, k]; total int64 [P, k]: sum C after every entry, exact"""
    for p, (o, V) in enumerate(zip(x_off, lens)):
        F = torch.round(x[o:o + V * V].view(V, V) * 2.0 ** 30).to(torch.int64)
        C = torch.full((V,), -2 ** 62, dtype=torch.int64, device=x.device)
        for j in range(k):
            s = torch.maximum(F, C).sum(1).argmax()
            C = torch.maximum(C, F.index_select(0, s.view(1))[0])
            second[p, j] = s
            total[p, j] = C.sum()                                  # int64: the host makes the coverage of it, outside the timing


def storyboard_table(N, v16, v8, s8, a):
    """One row per format: the two launches of `search.storyboard` over all videos of `cover_table`'s corpus in ONE pass (see the module
    docstring)"""
    from temporalalignnet_amd.search import align_tables, piece_offsets
    v_off = video_layouts(N)["corpus"]
    lens = np.diff(v_off.cpu().numpy().astype(np.int64))
    nv, k = len(lens), STORYBOARD_K
    s_off, first = piece_offsets(lens)
    hits, hit_off, x_off, table, n_x, sum_V = align_tables(lens, lens, first[:-1], np.arange(nv))
    dev = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr, dtype=dt)).cuda()        # noqa: E731
    s_off_d, hits_d, hit_off_d, x_off_d, table_d = dev(s_off, np.int32), dev(hits, np.int32), dev(hit_off, np.int64), dev(x_off, np.int64), \
        dev(table[:, 1:], np.int32)
    big = int(np.argmax(lens))
    one_off, one_table = dev([x_off[big]], np.int64), dev([[lens[big], 0]], np.int32)
    x = torch.empty(n_x, device="cuda")
    new = lambda n: (torch.empty(n, k, dtype=torch.int32, device="cuda"), torch.empty(n, k, device="cuda"))        # noqa: E731
    out, out_one = new(nv) + (torch.empty(sum_V, dtype=torch.int32, device="cuda"),), new(1) + (torch.empty(int(lens[big]), dtype=torch.int32, device="cuda"),)
    t_second, t_total = torch.empty(nv, k, dtype=torch.int32, device="cuda"), torch.empty(nv, k, dtype=torch.int64, device="cuda")
    rows = []
    for fmt in ("bf16", "e4m3"):
        feat, kw = (v16, {}) if fmt == "bf16" else (v8, dict(q_scale=s8, v_scale=s8))
        scores = lambda: ops.sequence_scores(feat, feat, s_off_d, v_off, hits_d, hit_off_d, x, **kw)             # noqa: E731
        select = lambda: ops.storyboard_select(x, x_off_d, table_d, k, sum_V=sum_V, out=out)                    # noqa: E731
        alone = lambda: ops.storyboard_select(x, one_off, one_table, k, sum_V=int(lens[big]), out=out_one)      # noqa: E731
        compose = lambda: torch_storyboard(x, x_off, lens, k, t_second, t_total)                                  # noqa: E731
        t_scores, _ = timed(scores, a.warmup, a.reps)
        t_sel, t_torch = timed_pair(select, compose, a.warmup, a.reps)
        s_a, s_b = timed_pair(select, select, a.warmup, a.reps)
        t_alone, _ = timed(alone, a.warmup, a.reps)
        # coverage of the composition's exact sums by the header's formula: int64 -> f32 to nearest even, * 2^-30, ONE f32 division
        want_cov = (t_total.cpu().numpy().astype(np.float32) * np.float32(2.0 ** -30)) / lens.astype(np.float32)[:, None]
        same_s = bool(torch.equal(out[0], t_second))
        same_c = bool(np.array_equal(out[1].cpu().numpy().view(np.int32), want_cov.view(np.int32)))
        gbs = k * float((lens * lens).sum()) * 4 / t_sel / 1e6
        rows.append({"fmt": fmt, "videos": nv, "sum_V2": int((lens * lens).sum()), "scores_ms": round(t_scores, 4), "select_ms": round(t_sel, 4),
                     "torch_ms": round(t_torch, 4), "select_over_torch": round(t_sel / t_torch, 5), "self_pair_spread": round(abs(s_a / s_b - 1), 4),
                     "equals_torch": same_s and same_c, "same_seconds": same_s, "same_coverage": same_c, "select_GBs": round(gbs, 1), "of_stream": round(gbs / (STREAM_TBS * 1e3), 4),
                     "longest_V": int(lens[big]), "longest_alone_ms": round(t_alone, 4)})
    return rows


CHAPTER_K, CHAPTER_MIN_LEN, CHAPTER_PENALTY = 12, 5, 0.05


def torch_chapter_costs(x, x_off, lens, cost):
    """What a caller writes without tan_chapter_costs, from the same blocks: per video fix(X) in int64, two cumsums, the four-corner
    difference and torch.div(..., rounding_mode="floor"); J(s, e) lands at [e - 1][s] of the video's block of `cost` (the other half
    holds whatever the triangle-blind expression gives); no host round trip"""
    for o, V in zip(x_off, lens):
        F = torch.round(x[o:o + V * V].view(V, V) * 2.0 ** 30).to(torch.int64)
        S = torch.zeros(V + 1, V + 1, dtype=torch.int64, device=x.device)
        S[1:, 1:] = F.cumsum(0).cumsum(1)
        d = torch.zeros(V + 1, dtype=torch.int64, device=x.device)
        d[1:] = F.diagonal().cumsum(0)
        diag = S.diagonal()
        ends = torch.arange(V + 1, device=x.device)
        n = (ends[:, None] - ends[None, :]).clamp(min=1)               # at [e, s]: e - s
        Q = diag[:, None] - S - S.T + diag[None, :]                    # at [e, s]: S[e,e] - S[e,s] - S[s,e] + S[s,s]
        J = (d[:, None] - d[None, :]) - torch.div(Q, n, rounding_mode="floor")
        cost[o:o + V * V].view(V, V).copy_(J[1:, :V])


def torch_chapter_decode(cost, x_off, lens, k, min_len, final):
    """... and without tan_chapter_decode: per video and level `(dp[None, :] + J).min(1)` over the allowed starts, in int64; final
    int64 [P, k]: dp_j[V] per level (2^62 where infeasible), from which count and scatter follow; no argument, no backtrack (the
    kernel does both), no host round trip inside a video"""
    INF = 2 ** 62
    for p, (o, V) in enumerate(zip(x_off, lens)):
        J = cost[o:o + V * V].view(V, V)                               # [e - 1, s]
        ends = torch.arange(1, V + 1, device=cost.device)
        starts = torch.arange(V, device=cost.device)
        allowed = (starts[None, :] >= 1) & (starts[None, :] <= ends[:, None] - min_len)
        dp = torch.full((V + 1,), INF, dtype=torch.int64, device=cost.device)
        dp[1:] = torch.where((ends >= min_len) | (ends == V), J[:, 0], dp[1:])
        final[p, 0] = dp[V]
        for j in range(1, k):
            cand = torch.where(allowed & (dp[None, :V] < INF), dp[None, :V] + J, torch.full_like(J, INF))
            dp = torch.cat((dp[:1], cand.min(1).values))
            final[p, j] = dp[V]


def chapters_table(N, v16, v8, s8, a):
    """One row per format: the launches of `search.chapters` over all videos of `cover_table`'s corpus in ONE pass (see the module
    docstring)"""
    from temporalalignnet_amd.search import align_tables, piece_offsets
    v_off = video_layouts(N)["corpus"]
    lens = np.diff(v_off.cpu().numpy().astype(np.int64))
    nv, k, min_len = len(lens), CHAPTER_K, CHAPTER_MIN_LEN
    s_off, first = piece_offsets(lens)
    hits, hit_off, x_off, table, n_x, sum_V = align_tables(lens, lens, first[:-1], np.arange(nv))
    dev = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr, dtype=dt)).cuda()        # noqa: E731
    s_off_d, hits_d, hit_off_d, x_off_d, table_d = dev(s_off, np.int32), dev(hits, np.int32), dev(hit_off, np.int64), dev(x_off, np.int64), \
        dev(table[:, 1:], np.int32)
    big = int(np.argmax(lens))
    one_off, one_table = dev([x_off[big]], np.int64), dev([[lens[big], 0]], np.int32)
    x = torch.empty(n_x, device="cuda")
    cost, t_cost = torch.empty(n_x, dtype=torch.int64, device="cuda"), torch.empty(n_x, dtype=torch.int64, device="cuda")
    new = lambda n, sv: (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, k, dtype=torch.int32, device="cuda"),   # noqa: E731
                         torch.empty(n, k, device="cuda"), torch.empty(sv, dtype=torch.int32, device="cuda"))
    out, out_one = new(nv, sum_V), new(1, int(lens[big]))
    ws = torch.empty(ops.chapter_decode_ws_bytes(nv, sum_V, k), dtype=torch.uint8, device="cuda")
    t_final = torch.empty(nv, k, dtype=torch.int64, device="cuda")
    levels = np.minimum(k, np.maximum(1, lens // min_len))
    read_bytes = float(((levels - 1) * lens * lens // 2).sum()) * 8
    lower = torch.zeros(n_x, dtype=torch.bool, device="cuda")
    for o, V in zip(x_off, lens):
        lower[o:o + V * V].view(V, V).copy_(torch.ones(V, V, dtype=torch.bool, device="cuda").tril())
    rows = []
    for fmt in ("bf16", "e4m3"):
        feat, kw = (v16, {}) if fmt == "bf16" else (v8, dict(q_scale=s8, v_scale=s8))
        ops.sequence_scores(feat, feat, s_off_d, v_off, hits_d, hit_off_d, x, **kw)
        costs = lambda: ops.chapter_costs(x, x_off_d, table_d, out=cost)                                          # noqa: E731
        t_costs = lambda: torch_chapter_costs(x, x_off, lens, t_cost)                                             # noqa: E731
        decode = lambda: ops.chapter_decode(cost, x_off_d, table_d, k, penalty=CHAPTER_PENALTY, min_len=min_len, sum_V=sum_V, out=out, ws=ws)   # noqa: E731
        t_decode = lambda: torch_chapter_decode(cost, x_off, lens, k, min_len, t_final)                           # noqa: E731
        one_costs = lambda: ops.chapter_costs(x, one_off, one_table, out=cost)                                    # noqa: E731
        one_decode = lambda: ops.chapter_decode(cost, one_off, one_table, k, penalty=CHAPTER_PENALTY, min_len=min_len,   # noqa: E731
                                                sum_V=int(lens[big]), out=out_one, ws=ws)
        c_new, c_torch = timed_pair(costs, t_costs, a.warmup, a.reps)
        c_a, c_b = timed_pair(costs, costs, a.warmup, a.reps)
        d_new, d_torch = timed_pair(decode, t_decode, a.warmup, a.reps)
        d_a, d_b = timed_pair(decode, decode, a.warmup, a.reps)
        same_costs = bool(torch.equal(cost[lower], t_cost[lower]))
        want = t_final.cpu().numpy()
        want_scatter = np.where(want < 2 ** 62, want.astype(np.float32) * np.float32(2.0 ** -30), np.float32(np.inf)).astype(np.float32)
        same_scatter = bool(np.array_equal(out[2].cpu().numpy().view(np.int32), want_scatter.view(np.int32)))
        t_one_c, _ = timed(one_costs, a.warmup, a.reps)
        t_one_d, _ = timed(one_decode, a.warmup, a.reps)
        sum_v2 = float((lens * lens).sum())
        c_gbs, d_gbs = sum_v2 * (4 + 4) / c_new / 1e6, read_bytes / d_new / 1e6                                   # costs: x in, half of cost out
        rows.append({"fmt": fmt, "videos": nv, "sum_V2": int(sum_v2), "costs_ms": round(c_new, 4), "torch_costs_ms": round(c_torch, 4),
                     "costs_over_torch": round(c_new / c_torch, 5), "costs_spread": round(abs(c_a / c_b - 1), 4), "same_costs": same_costs,
                     "costs_GBs": round(c_gbs, 1), "costs_of_stream": round(c_gbs / (STREAM_TBS * 1e3), 4),
                     "decode_ms": round(d_new, 4), "torch_decode_ms": round(d_torch, 4), "decode_over_torch": round(d_new / d_torch, 5),
                     "decode_spread": round(abs(d_a / d_b - 1), 4), "same_scatter": same_scatter, "decode_GBs": round(d_gbs, 1),
                     "chapters": int(out[0].sum()), "longest_V": int(lens[big]), "longest_costs_ms": round(t_one_c, 4),
                     "longest_decode_ms": round(t_one_d, 4)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def rerank_table(N, v16, stem, a):
    import time

    from temporalalignnet_amd import search
    from temporalalignnet_amd.tan_model import TemporalAligner
    torch.manual_seed(0)
    m = TemporalAligner(6, 6, use_alignability_head=1, random_pos_start=0, language_model=None, compute_dtype="bf16").cuda().eval()
    v_off = video_layouts(N)["corpus"]
    nv = v_off.numel() - 1
    idx = search.VideoIndex(v16, v_off.cpu().numpy(), [f"v{i}" for i in range(nv)], stem=stem)
    T, Kp, pool, wpp = 64, search.RERANK_TEXT_SLOTS, min(a.pool, nv), 256
    m._ensure_flat()
    hw, hb = m._f("binary_head.weight").view(-1), m._f("binary_head.bias")
    rows = []
    for Q in a.queries:
        emb = torch.randn(Q, 512, generator=torch.Generator(device="cuda").manual_seed(Q), device="cuda")
        tq = search.query_features(idx, m, lambda qs: emb, [""] * Q)
        out = (torch.empty(Q, pool, device="cuda"), torch.empty(Q, pool, dtype=torch.int32, device="cuda"),
               torch.empty(Q, pool, dtype=torch.int32, device="cuda"))
        ws = torch.empty(ops.rank_topk_video_ws_bytes(Q, N, nv, pool), dtype=torch.uint8, device="cuda")
        t_dual, _ = timed(lambda: ops.rank_topk_video(tq, v16, v_off, pool, out=out, ws=ws), a.warmup, a.reps)
        km = min(10, nv)
        mout = tuple(t[:, :km].contiguous() for t in out)
        ext = (torch.empty(Q, km, dtype=torch.int32, device="cuda"), torch.empty(Q, km, dtype=torch.int32, device="cuda"))

        def moments():
            ops.rank_topk_video(tq, v16, v_off, km, out=mout, ws=ws)
            ops.moment_extent(tq, v16, v_off, *mout, 0.07, out=ext)
        t_mom, _ = timed(moments, a.warmup, a.reps)
        ops.rank_topk_video(tq, v16, v_off, pool, out=out, ws=ws)
        table = search._rerank_table(v_off, out[1], out[2], T)
        n_win = Q * pool
        passes = [(p0, min(p0 + wpp, n_win)) for p0 in range(0, n_win, wpp)]
        W0 = passes[0][1]
        win = torch.empty(W0, T, 512, dtype=stem.dtype, device="cuda")
        vm, tm = torch.empty(W0, T, dtype=torch.bool, device="cuda"), torch.empty(W0, Kp, dtype=torch.bool, device="cuda")
        txt = torch.empty(W0, Kp, 512, device="cuda")
        res = torch.empty(n_win, 4, device="cuda")
        order = torch.empty(Q, min(10, pool), dtype=torch.int32, device="cuda")

        def joint():
            for p0, p1 in passes:
                W = p1 - p0
                ops.window_pack(stem, emb, table[p0:p1], T, Kp, win[:W], vm[:W], txt[:W], tm[:W])
                m._release_ws(m.joint_from_stem(win[:W], vm[:W], txt[:W], tm[:W]))
        t_joint, _ = timed(joint, a.warmup, a.reps)
        kept = {p1 - p0: None for p0, p1 in passes}
        for W in kept:                                            # a finished pass of each size: the tail's input
            ops.window_pack(stem, emb, table[:W], T, Kp, win[:W], vm[:W], txt[:W], tm[:W])
            kept[W] = m.joint_from_stem(win[:W], vm[:W], txt[:W], tm[:W])

        def tail():
            for p0, p1 in passes:
                ej = kept[p1 - p0]
                ops.rerank_tail(ej.stage(5), ej.stage(2), table[p0:p1], T, hw, hb, res[p0:p1])
            ops.rerank_select(res.view(Q, pool, 4), order.shape[1], stride=4, out=order)
        t_tail, _ = timed(tail, a.warmup, a.reps)
        for ej in kept.values():
            m._release_ws(ej)

        def end_to_end():
            t0 = time.perf_counter()
            search.search_rerank(idx, m, lambda qs: emb, [""] * Q, k=order.shape[1], pool=pool, windows_per_pass=wpp)
            return (time.perf_counter() - t0) * 1e3
        for _ in range(a.warmup):
            end_to_end()
        t_e2e = float(np.median([end_to_end() for _ in range(a.reps)]))
        raw = torch.randn(W0, T, 1024, generator=torch.Generator(device="cuda").manual_seed(7), device="cuda").abs()
        vm.zero_()
        tm.fill_(True)
        tm[:, 0] = False

        def evalw():
            for p0, p1 in passes:
                W = p1 - p0
                m.eval_windows(raw[:W], txt[:W], vm[:W], tm[:W])
        t_eval, _ = timed(evalw, a.warmup, a.reps)
        rows.append({"Q": Q, "pool": pool, "videos": nv, "windows": n_win, "passes": len(passes), "dual_ms": round(t_dual, 4),
                     "joint_ms": round(t_joint, 4), "tail_select_ms": round(t_tail, 4),
                     "stages_ms": round(t_dual + t_joint + t_tail, 4), "end_to_end_ms": round(t_e2e, 4),
                     "moments_ms": round(t_mom, 4), "eval_windows_ms": round(t_eval, 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 * 2 ** 20)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--moments", action="store_true", help="also time rank_topk_video and moment_extent (see the module docstring)")
    ap.add_argument("--sequences", action="store_true", help="time sequence_topk against the video and row sweeps instead (see the module docstring)")
    ap.add_argument("--clips", action="store_true", help="time clip_topk against sequence_topk and the row sweep instead (see the module docstring)")
    ap.add_argument("--copies", action="store_true",
                    help="time local_align against monotonic_decode and the host restatement, and search_copies, instead (see the module docstring)")
    ap.add_argument("--rerank", action="store_true", help="time the stages of search_rerank instead (see the module docstring)")
    ap.add_argument("--pool", type=int, default=32)
    ap.add_argument("--shards", type=int, nargs="?", const=8, default=0, metavar="S",
                    help="time sharded search over S shards (default 8) instead (see the module docstring)")
    ap.add_argument("--restrict", action="store_true", help="time the filtered sweep instead (see the module docstring)")
    ap.add_argument("--paths-out", default=None, metavar="FILE", help="with --copies: write the local_align_path table here")
    ap.add_argument("--parent-lib", default=None, metavar="PATH",
                    help="with --restrict: libtan_hip.so of the parent commit's build, whose plain sweep is timed in the same run; "
                         "with --copies: its tan_local_align is timed twice beside this build's; "
                         "with --annotate: its sweep checks that this build's route (a) is the parent's")
    ap.add_argument("--annotate", action="store_true", help="time label_topk and label_runs instead (see the module docstring)")
    ap.add_argument("--labels", type=int, nargs="+", default=[128, 1024, 8192], help="with --annotate: vocabulary sizes")
    ap.add_argument("--annotate-k", type=int, nargs="+", default=list(ANNOTATE_KS), help="with --annotate: labels kept per row")
    ap.add_argument("--storyboard", action="store_true", help="time storyboard_select and its score blocks instead (use --rows 1048576)")
    ap.add_argument("--chapters", action="store_true", help="time chapter_costs and chapter_decode against their torch compositions instead "
                                                            "(use --rows 1048576)")
    ap.add_argument("--cover", action="store_true", help="time cover_topk against label_topk(k = 1) at L = m instead (use --rows 1048576)")
    ap.add_argument("--cover-rows", type=int, nargs="+", default=[128, 1024, 4096], help="with --cover: rows of the one set")
    a = ap.parse_args()
    N, k = a.rows, a.k
    if a.rerank:
        if a.queries == [1, 64, 1024]:
            a.queries = [1, 64]
        v16 = torch.empty(N, 512, dtype=torch.bfloat16, device="cuda")
        stem = torch.empty(N, 512, dtype=torch.bfloat16, device="cuda")
        for r in range(0, N, SLICE):
            v16[r:r + SLICE] = unit_rows(min(SLICE, N - r), r).to(torch.bfloat16)
            stem[r:r + SLICE] = (unit_rows(min(SLICE, N - r), N + r) * 4).to(torch.bfloat16)
        rows = rerank_table(N, v16, stem, a)
        res = {"rows": N, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "rerank": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --rerank --rows {N} --pool {a.pool}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
                fh.write("# bf16 index + bf16 stem, 6 + 6 layer bf16 model with the head, passes of 256 windows of 64 s; stages_ms = dual + joint + "
                         "tail_select (device events); end_to_end_ms = search_rerank on the host clock; moments_ms = rank_topk_video + moment_extent "
                         "at k = 10; eval_windows_ms = eval_windows over as many raw-feature windows (both stacks)\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>15}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>15}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    v16 = torch.empty(N, 512, dtype=torch.bfloat16, device="cuda")
    v8 = torch.empty(N, 512, dtype=torch.uint8, device="cuda")
    s8 = torch.empty(N, device="cuda")
    for r in range(0, N, SLICE):
        x = unit_rows(min(SLICE, N - r), r)
        v16[r:r + SLICE] = x.to(torch.bfloat16)
        ops.quantize_rows_e4m3(x, v8[r:r + SLICE], s8[r:r + SLICE])
    del x
    if a.storyboard:
        rows = storyboard_table(N, v16, v8, s8, a)
        res = {"rows": N, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "storyboard": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --storyboard --rows {N}: median of {a.reps} after {a.warmup} warm-ups, device events, caller-owned "
                         f"outputs, {res['gpu']}\n")
                fh.write(f"# all videos (60 to 1 200 rows) in one pass, k = {STORYBOARD_K}; scores = ops.sequence_scores, the index's own rows as the "
                         "queries; select = ops.storyboard_select over its blocks; torch = per video k iterations of "
                         "torch.maximum(fix(X), C).sum(1).argmax() in int64 from the same blocks, alternating call by call with select; "
                         "self_pair_spread = |ratio - 1| of select alternating with itself; select_GBs = k sum_V2 4 bytes / select time, of_stream: of "
                         f"{STREAM_TBS} TB/s; longest_alone = select over the longest video alone (one workgroup)\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>17}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>17}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    if a.chapters:
        rows = chapters_table(N, v16, v8, s8, a)
        res = {"rows": N, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "chapters": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --chapters --rows {N}: median of {a.reps} after {a.warmup} warm-ups, device events, caller-owned "
                         f"outputs, {res['gpu']}\n")
                fh.write(f"# all videos (60 to 1 200 rows) in one pass, k = {CHAPTER_K}, min_len = {CHAPTER_MIN_LEN}, penalty = {CHAPTER_PENALTY}; costs = "
                         "ops.chapter_costs over tan_sequence_scores' blocks, decode = ops.chapter_decode over its costs; torch_* = what a caller "
                         "writes without them from the same blocks (per video: fix(X) in int64, two cumsums, the four-corner difference, "
                         "torch.div floor; per level (dp[None, :] + J).min(1)), alternating call by call with the kernel; *_spread = |ratio - 1| "
                         "of the kernel alternating with itself; costs_GBs = sum_V2 * 8 bytes (x in, half of cost out) / costs time, of_stream: "
                         f"of {STREAM_TBS} TB/s; decode_GBs = sum (levels - 1) V^2 / 2 * 8 bytes / decode time; longest_* = the longest video alone\n")
                for r in rows:
                    for c in r:
                        fh.write(f"{r['fmt']:>5} {c:>20} {r[c]}\n")
        print(json.dumps(res))
        return
    if a.cover:
        rows = cover_table(N, v16, v8, s8, a)
        res = {"rows": N, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "cover": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --cover --rows {N}: median of {a.reps} after {a.warmup} warm-ups, device events, caller-owned "
                         f"outputs, {res['gpu']}\n")
                fh.write("# cover_topk = ops.cover_topk of one set of m random unit rows over all rows, videos of 60 to 1 200 rows, rank both, "
                         "k = 10; label_topk = ops.label_topk(k = 1) with the set as L = m labels over the same rows, the two alternating call by "
                         "call; self_pair_spread = |ratio - 1| of cover_topk alternating with itself; TFLOPs = 2 N m 512 / cover_topk time\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>17}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>17}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    if a.annotate:
        rows = annotate_table(N, v16, v8, s8, a)
        res = {"rows": N, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "annotate": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --annotate --rows {N}: median of {a.reps} after {a.warmup} warm-ups, device events, caller-owned "
                         f"outputs, {res['gpu']}\n")
                fh.write(f"# label_topk = ops.label_topk over all rows; swapped_rank = ops.rank_topk with the rows as queries and the labels as the "
                         f"index over chunks of {ANNOTATE_CHUNK} rows, the two alternating call by call; self_pair_spread = |ratio - 1| of label_topk "
                         "alternating with itself; torch = matmul + topk over the same chunks (bf16); TFLOPs = 2 N L 512 / label_topk time; "
                         f"of_bf16_mfma_peak against {BF16_MFMA_PEAK_TF / 1000} PF (specification); label_stream = ceil(N / 128) x L x row bytes / "
                         f"time, against {L2_SHARED_TBS[0]}-{L2_SHARED_TBS[1]} TB/s (rows shared by an XCD's workgroups, from L2) and "
                         f"{INF_CACHE_TBS} TB/s (Infinity Cache): figures of the microarchitecture notes the design assumed, not measurements of "
                         "this kernel; runs = ops.label_runs at the median best score (about half the rows kept); decode = ops.label_decode over "
                         f"the same lists at that threshold and penalty {DECODE_SWITCH}, videos of 60 to 1 200 rows, one wave per video; "
                         f"decode_stream = (N k 8 + 2 N (k + 1) + N 8) bytes at {HBM_COPY_TBS} TB/s\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>21}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>21}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    if a.restrict:
        rows = restrict_table(N, k, v16, v8, s8, a)
        res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "restrict": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --restrict --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
                fh.write(f"# {N // RESTRICT_VLEN} videos of {RESTRICT_VLEN} rows, whole videos drawn uniformly (fixed seed); build = row_filter_build; "
                         "filtered = rank_topk_filtered; plain = rank_topk over the whole index, parent_plain = the parent commit's build of it, "
                         "alternating call by call; gather = index_select of the admitted rows + rank_topk over them\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>22}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>22}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    if a.shards:
        rows = shards_table(N, k, v16, v8, s8, a)
        res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "shards": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --shards {a.shards} --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
                fh.write("# single = one rank_topk sweep; device_shards = a sweep + a tan_topk_fold per device-resident shard; host_shards = the same "
                         "with the shards streamed from pinned host memory through two slots (GB/s of index bytes); copy = plain pinned copy_ of "
                         "the same bytes into one slot, same run\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>18}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>18}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    if a.copies:
        del v8, s8
        rows, e2e, paths = copies_table(N, k, v16, a)
        res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "copies": rows, "search": e2e,
               "paths": paths}
        if a.paths_out:
            os.makedirs(os.path.dirname(os.path.abspath(a.paths_out)), exist_ok=True)
            with open(a.paths_out, "w") as fh:
                fh.write(f"# tools/search_bench.py --copies --rows {N}: median of {a.reps} after {a.warmup} warm-ups, device events, caller-owned "
                         f"outputs and scratch, {res['gpu']}\n")
                fh.write(f"# local_align_path (the time map) beside local_align over the same blocks (threshold {ALIGN_PRICES[0]}, skew "
                         f"{ALIGN_PRICES[1]}, scores N(0, 1/512)), alternating call by call; trace = 16 bytes x ceil(m / 64) x (V + 63) per block; "
                         "read_back = what a caller copies to the host (score, span; + 8 bytes per query second); parent_align / parent_again = "
                         "--parent-lib's tan_local_align twice in the same round, parent_spread = the distance of its two medians\n")
                cols = list(paths[0])
                fh.write(" ".join(f"{c:>21}" for c in cols) + "\n")
                for r in paths:
                    fh.write(" ".join(f"{str(r[c]):>21}" for c in cols) + "\n")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --copies --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
                fh.write(f"# local_align (threshold {ALIGN_PRICES[0]}, skew {ALIGN_PRICES[1]}, scores N(0, 1/512)) against monotonic_decode over the "
                         "same blocks (device events) and the host path: read_back = x.cpu(), host_ref = the float32 numpy restatement over "
                         "host_blocks blocks (host clock), host_scaled = read_back + host_ref * P / host_blocks; the three alternate call by "
                         "call; steps = ceil(m / 64) * (V + 63) anti-diagonals per block\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>19}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>19}" for c in cols) + "\n")
                fh.write("# end to end, bf16 index, host clock around calls that end in their read-back: search_copies (40 s query, pool 32, "
                         "piece 16, threshold 0.4, skew 0.1) beside search_clips (its first 32 s)\n")
                fh.write(" ".join(f"{c:>19}" for c in e2e) + "\n")
                fh.write(" ".join(f"{str(v):>19}" for v in e2e.values()) + "\n")
        print(json.dumps(res))
        return
    if a.clips:
        def idx_of(q):
            q8, qs8 = ops.quantize_rows_e4m3(q)
            return {"bf16": (q.to(torch.bfloat16), v16, {}), "e4m3": (q8, v8, dict(q_scale=qs8, v_scale=s8))}
        rows = clips_table(N, k, idx_of, a)
        res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "clips": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --clips --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
                fh.write("# clip_topk against sequence_topk (the same clips as sequences) and rank_topk with Q = n_clip * m queries, same run, "
                         "same rows\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>14}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>14}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    if a.sequences:
        def idx_of(q):
            q8, qs8 = ops.quantize_rows_e4m3(q)
            return {"bf16": (q.to(torch.bfloat16), v16, {}), "e4m3": (q8, v8, dict(q_scale=qs8, v_scale=s8))}
        rows = sequences_table(N, k, idx_of, a)
        res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "sequences": rows}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(f"# tools/search_bench.py --sequences --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
                fh.write("# sequence_topk against rank_topk_video and rank_topk with Q = n_seq * m queries, same run, same rows; finish_ms = "
                         "sequence_scores + monotonic_decode for the n_seq * k winners\n")
                cols = list(rows[0])
                fh.write(" ".join(f"{c:>18}" for c in cols) + "\n")
                for r in rows:
                    fh.write(" ".join(f"{str(r[c]):>18}" for c in cols) + "\n")
        print(json.dumps(res))
        return
    rows = []
    for Q in a.queries:
        q = unit_rows(Q, 1 << 30)
        q16 = q.to(torch.bfloat16)
        q8, qs8 = ops.quantize_rows_e4m3(q)
        ws = torch.empty(ops.rank_topk_ws_bytes(Q, N, k), dtype=torch.uint8, device="cuda")
        out = (None, None, torch.empty(Q, k, device="cuda"), torch.empty(Q, k, dtype=torch.int32, device="cuda"))
        t16, b16 = timed(lambda: ops.rank_topk(q16, v16, None, k, out=out, ws=ws), a.warmup, a.reps)
        top16 = out[3].clone()
        t8, b8 = timed(lambda: ops.rank_topk_e4m3(q8, qs8, v8, s8, None, k, out=out, ws=ws), a.warmup, a.reps)
        agree = float((top16[:, 0] == out[3][:, 0]).float().mean())
        by16, by8 = N * 1024, N * 516
        rows.append({"Q": Q, "bf16_ms": round(t16, 4), "bf16_min_ms": round(b16, 4), "e4m3_ms": round(t8, 4), "e4m3_min_ms": round(b8, 4),
                     "e4m3_over_bf16": round(t8 / t16, 3),
                     "bf16_TBps": round(by16 / t16 * 1e-9, 3), "e4m3_TBps": round(by8 / t8 * 1e-9, 3),
                     "bf16_of_stream": round(by16 / t16 * 1e-9 / STREAM_TBS, 3), "e4m3_of_stream": round(by8 / t8 * 1e-9 / STREAM_TBS, 3),
                     "bf16_TFLOPs": round(2.0 * Q * N * 512 / t16 * 1e-9, 1), "e4m3_TFLOPs": round(2.0 * Q * N * 512 / t8 * 1e-9, 1),
                     "top1_agree": round(agree, 4)})
        if a.moments:
            idx = {"bf16": (q16, v16, {}), "e4m3": (q8, v8, dict(q_scale=qs8, v_scale=s8))}
            rows[-1].update(moments_row(Q, N, k, idx, {"bf16": t16, "e4m3": t8}, a))
    res = {"rows": N, "k": k, "reps": a.reps, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0), "stream_TBps": STREAM_TBS,
           "table": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(f"# tools/search_bench.py --rows {N} -k {k}: median of {a.reps} after {a.warmup} warm-ups, {res['gpu']}\n")
            fh.write(f"# index bytes per sweep: bf16 {N * 1024}, e4m3 {N * 516}; of_stream = bytes/s over {STREAM_TBS} TB/s\n")
            cols = [c for c in rows[0] if not c.startswith(("corpus_", "one_"))]
            fh.write(" ".join(f"{c:>15}" for c in cols) + "\n")
            for r in rows:
                fh.write(" ".join(f"{r[c]:>15}" for c in cols) + "\n")
            if a.moments:
                fh.write("# --moments: rank_topk_video / moment_extent (width 0.07) per v_off layout; video_over_rows = video sweep ms over "
                         "rank_topk ms above\n")
                cols = ["layout", "fmt", "Q", "videos", "k", "video_ms", "video_over_rows", "extent_ms", "moment_rows"]
                fh.write(" ".join(f"{c:>15}" for c in cols) + "\n")
                for name in ("corpus", "one"):
                    for fmt in ("bf16", "e4m3"):
                        for r in rows:
                            vals = [name, fmt, r["Q"], r[f"{name}_videos"], r[f"{name}_k"]] + [r[f"{name}_{fmt}_{c}"] for c in cols[5:]]
                            fh.write(" ".join(f"{v:>15}" for v in vals) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
