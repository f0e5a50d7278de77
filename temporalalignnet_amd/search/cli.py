"""The command line (`python -m temporalalignnet_amd.search`; synopsis: the package docstring): one parser, and per subcommand one
function that checks its arguments (`_check_*`, argparse errors: exit code 2) and one that runs it (`_run_*`: the exit code)."""
import argparse
import sys

import numpy as np
import torch

from . import __doc__ as _PACKAGE_DOC                # its first paragraph is the parser's description
from ..infer_align import build_aligner, make_embed_text, read_corpus
from .annotation import annotate, write_per_second_csv, write_segments_csv
from .cluster import MAX_CLUSTERS, StepClusters, discover_steps
from .coarse import CoarseImage
from .index import E4M3, ShardedIndex, VideoIndex, build_index
from .summary import (MAX_CHAPTER_K, MAX_CHAPTER_SECONDS, MAX_STORYBOARD_K, MAX_STORYBOARD_SECONDS, chapters, storyboard,
                      write_chapters_csv, write_storyboard_csv)
from .text import TEMPERATURE, Compound, search, search_compound, search_moments, search_rerank, search_sequences
from .video import MAX_ALIGN_SECONDS, MAX_CLIP_SECONDS, MAX_COVER_SECONDS, search_clips, search_copies, search_cover


def _parser():
    # prog: the usage line of `python -m temporalalignnet_amd.search` as it has always read, not "__main__.py"
    ap = argparse.ArgumentParser(prog="search.py", description=_PACKAGE_DOC.split("\n\n")[0],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("index", "query", "annotate"):
        _model_options(sub.add_parser(name), required=name != "annotate")      # annotate --clusters takes no model
    p = sub.choices["index"]
    p.add_argument("--feature-dir", required=True)
    p.add_argument("--asr-json", required=True)
    p.add_argument("--vlen-csv", required=True)
    p.add_argument("--out", required=True, help="index file (.npz)")
    p.add_argument("--index-dtype", choices=("bf16", "fp32", "e4m3"), default=None,
                   help="row format of the index (default: --dtype); e4m3: 516 bytes per second instead of 1 KiB")
    p.add_argument("--keep-stem", action="store_true",
                   help="also keep video_pre_proj of every second (what `query --rerank` needs): + 1 KiB per second in bf16")
    p.add_argument("--worker-id", type=int, default=0)
    p.add_argument("--num-workers", type=int, default=1)
    for name in ("query", "annotate"):
        _index_options(sub.choices[name])
    p = sub.choices["annotate"]
    p.add_argument("--labels", default=None, metavar="FILE", help="the vocabulary: one label text per line, blank lines skipped")
    p.add_argument("--clusters", default=None, metavar="FILE",
                   help="in --labels' place: the steps `discover` found (its --out), for this or another index; no checkpoint needed")
    p.add_argument("-k", type=int, default=1, help="labels kept per second, 1 to 32 (segments use the best one)")
    p.add_argument("--threshold", type=float, default=None,
                   help="a second whose best score is below this is background (default: none is)")
    p.add_argument("--min-len", type=int, default=None, help="drop segments shorter than this many seconds (default 1)")
    p.add_argument("--smooth", type=float, default=None, metavar="PENALTY",
                   help="decode every video's labels with this penalty per label change (>= 0; needs a finite --threshold, "
                        "use -k 5 or more): segments bridge short dips and flickers")
    p.add_argument("--per-second", action="store_true", help="write vid,second,label,score for the k labels of every second instead")
    p.add_argument("--out", required=True, metavar="CSV", help="vid,start,end,label,peak,score: one row per segment")
    p = sub.choices["query"]
    p.add_argument("-k", type=int, default=10)
    p.add_argument("--moments", action="store_true",
                   help="the k best distinct videos, each as `sentence vid start end second score` (seconds of the video)")
    p.add_argument("--width", type=float, default=None,
                   help=f"with --moments: a moment extends while the score stays within this of its peak (default {TEMPERATURE})")
    p.add_argument("--sequence", action="store_true",
                   help="the sentences are ONE ordered list of steps: the k videos that show them in order, each as "
                        "`vid score t_0 ... t_{m-1}` (seconds of the video, non-decreasing)")
    p.add_argument("--all", action="store_true", dest="all_",
                   help="the sentences are the clauses of ONE compound query, `|` between a clause's alternatives: the k videos that "
                        "show every clause in whatever order, each as `vid score second:peak ...` (one pair per sentence, "
                        "alternatives in place, then the --none ones)")
    p.add_argument("--none", action="extend", nargs="+", default=None, metavar="S",
                   help="with --all: a video where one of these sentences peaks at --veto or above is left out")
    p.add_argument("--veto", type=float, default=None, help="with --none: the peak that bans a video (no default: its scale is the model's)")
    p.add_argument("--rerank", action="store_true",
                   help="two stages: the --pool best distinct videos of the dual sweep rescored by the joint encoder, the k best as "
                        "`sentence vid second score confidence alignability dual_second dual_score` (needs index --keep-stem)")
    p.add_argument("--pool", type=int, default=None,
                   help="with --rerank: candidates per sentence, 1 to 32 (default 32); with --coarse: any number >= 1 (default 64)")
    p.add_argument("--coarse", default=None, metavar="FILE",
                   help="the index's coarse image (what `coarse` writes): it proposes --pool candidates per sentence on the card and "
                        "only their full rows are scored exactly -- for a --host-resident index no shard crosses the host link")
    p.add_argument("--only", action="append", default=None, metavar="VID", help="search only this video (repeatable)")
    p.add_argument("--only-file", default=None, metavar="PATH", help="search only the videos listed here, one vid per line")
    p.add_argument("--exclude", action="append", default=None, metavar="VID", help="leave this video out (repeatable)")
    p.add_argument("--exclude-file", default=None, metavar="PATH", help="leave out the videos listed here, one vid per line")
    p.add_argument("--within", action="append", default=None, metavar="VID:FIRST-LAST",
                   help="search this video only between these seconds, inclusive (repeatable; other videos stay whole)")
    p.add_argument("sentences", nargs="+")
    p = sub.add_parser("similar", help="where else in the corpus a piece of an indexed video appears (no checkpoint, no model)")
    _index_options(p)
    p.add_argument("--clip", action="append", required=True, metavar="VID:FIRST-LAST",
                   help=f"these seconds of this video of the index, inclusive, at most {MAX_CLIP_SECONDS} (repeatable)")
    p.add_argument("-k", type=int, default=10)
    p.add_argument("--keep-source", action="store_true", help="also list the video the clip was cut from (left out by default)")
    p.add_argument("--align", action="store_true",
                   help=f"find re-timed or re-cut copies: the best local alignment of the clip (then up to {MAX_ALIGN_SECONDS} seconds) "
                        "with each candidate video, as `vid start end score q_start q_end cells` (needs --threshold)")
    p.add_argument("--threshold", type=float, default=None,
                   help="with --align: a second of the alignment gains its score minus this (no default: it depends on the features)")
    p.add_argument("--skew", type=float, default=None, help="with --align: the price of a step along one video alone, >= 0 (default 0)")
    p.add_argument("--pool", type=int, default=None, help="with --align: candidate videos per piece, 1 to 32 (default 32)")
    p.add_argument("--piece", type=int, default=None,
                   help=f"with --align: the clip is cut into pieces of this many seconds for the candidate sweep, 1 to {MAX_CLIP_SECONDS} "
                        "(default 16)")
    p.add_argument("--map", default=None, metavar="OUT.csv",
                   help="with --align: write the time map of every hit, one row `query,vid,query_second,first,last` per aligned second "
                        "of the clip (query_second on the clip's own video timeline; first..last the seconds of vid that show it)")
    p.add_argument("--cover", action="store_true",
                   help=f"rank videos by the seconds they share with the clip (then up to {MAX_COVER_SECONDS} seconds) in any order and "
                        "at any pace, as `vid score forward backward`")
    p.add_argument("--rank", choices=("both", "query", "video"), default=None,
                   help="with --cover: rank by how much of the clip is in the video (query), how much of the video is in the clip "
                        "(video), or the mean of the two (both, the default)")
    p = sub.add_parser("discover", help="which steps recur in the corpus: cluster the index's seconds (no checkpoint, no vocabulary)")
    _index_options(p)
    _model_options(p, required=False)
    p.add_argument("-k", type=int, required=True, help=f"clusters, 1 to {MAX_CLUSTERS}")
    p.add_argument("--iters", type=int, default=10, help="centroid updates at most (default 10); stops early when no second moves")
    p.add_argument("--seed", type=int, default=0, help="of the k seconds the centroids start from")
    p.add_argument("--out", required=True, metavar="FILE", help="the clusters (.npz), what `annotate --clusters` takes")
    p.add_argument("--exemplars", type=int, default=None, metavar="N", help="also print every cluster's N best seconds, 1 to 32")
    p.add_argument("--labels", default=None, metavar="FILE",
                   help="name every cluster by the nearest line of this vocabulary (needs --checkpoint and --vocab)")
    p.add_argument("--segments", default=None, metavar="CSV", help="also write the clustered index's segments, as `annotate` does")
    p.add_argument("--threshold", type=float, default=None, help="with --segments: a second scoring below this is background")
    p.add_argument("--min-len", type=int, default=None, help="with --segments: drop segments shorter than this many seconds")
    p.add_argument("--smooth", type=float, default=None, metavar="PENALTY",
                   help="with --segments: decode every video's steps with this penalty per change (needs a finite --threshold)")
    p = sub.add_parser("coarse", help="the MXFP4 image of an index, 272 bytes per second: what `query --coarse` takes (no checkpoint)")
    _index_options(p)
    p.add_argument("--out", required=True, metavar="FILE", help="the image (.npz)")
    p = sub.add_parser("storyboard", help="the k seconds that best summarise each video (no checkpoint, no model)")
    _index_options(p)
    p.add_argument("-k", type=int, default=8, help=f"seconds per video at most, 1 to {MAX_STORYBOARD_K} (default 8)")
    p.add_argument("--min-gain", type=float, default=None, metavar="X",
                   help="stop a video's selection when the next second would raise its mean coverage by less than this (default 0: "
                        "only when it would add nothing)")
    p.add_argument("--only", action="append", default=None, metavar="VID", help="only this video (repeatable)")
    p.add_argument("--only-file", default=None, metavar="PATH", help="only the videos listed here, one vid per line")
    p.add_argument("--skip-long", action="store_true",
                   help=f"leave out videos of more than {MAX_STORYBOARD_SECONDS} seconds instead of refusing them")
    p.add_argument("--out", required=True, metavar="CSV", help="vid,rank,second,coverage,share: one row per chosen second")
    p.add_argument("--npz", default=None, metavar="FILE", help="also save the storyboard (seconds, coverage, owners) as .npz")
    p = sub.add_parser("chapters", help="cut each video into contiguous chapters (no checkpoint, no model)")
    _index_options(p)
    p.add_argument("-k", type=int, default=12, help=f"chapters per video at most, 1 to {MAX_CHAPTER_K} (default 12)")
    p.add_argument("--penalty", type=float, required=True, metavar="X",
                   help="keep a boundary only if it lowers the summed within-chapter scatter by at least this much (score x seconds; "
                        "no default: its scale is the model's)")
    p.add_argument("--min-len", type=int, default=None, metavar="M", help="seconds per chapter at least (default 1)")
    p.add_argument("--only", action="append", default=None, metavar="VID", help="only this video (repeatable)")
    p.add_argument("--only-file", default=None, metavar="PATH", help="only the videos listed here, one vid per line")
    p.add_argument("--skip-long", action="store_true",
                   help=f"leave out videos of more than {MAX_CHAPTER_SECONDS} seconds instead of refusing them")
    p.add_argument("--out", required=True, metavar="CSV", help="vid,chapter,start,end,seconds: one row per chapter")
    p.add_argument("--npz", default=None, metavar="FILE", help="also save the chapters (starts, scatter, per-second numbers) as .npz")
    p = sub.add_parser("merge", help="concatenate index files into one (no checkpoint, no GPU)")
    p.add_argument("--out", required=True, help="index file (.npz)")
    p.add_argument("inputs", nargs="+", help="index files, in the order their videos get")
    return ap


def _model_options(p, required=True):
    """--checkpoint --vocab [--dtype] [--model]: the aligner of `index`, `query`, `annotate --labels` and `discover --labels`"""
    p.add_argument("--checkpoint", required=required, default=None)
    p.add_argument("--vocab", required=required, default=None, help="s3d_dict.npy (the Word2Vec vocabulary)")
    p.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    p.add_argument("--model", choices=("init", "cotrain"), default="init")


def _index_options(p):
    """--index [--shard ...] [--host-resident]: what `query`, `annotate` and `similar` load their index from (`_load_index`)"""
    p.add_argument("--index", required=True)
    p.add_argument("--shard", action="append", default=None, metavar="PATH",
                   help="a further index file searched together with --index, in the order given (repeatable)")
    p.add_argument("--host-resident", action="store_true",
                   help="keep the rows in pinned host memory and stream them through the card: for an index larger than the card")


def parse_args(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    _CHECKS[a.cmd](ap, a)
    return a


def _refuse(ap, *cases):
    """`ap.error` (exit code 2) with the text of the first case (holds, text) that holds"""
    for holds, text in cases:
        if holds:
            ap.error(text)


def _check_index(ap, a):
    _refuse(ap, (not 0 <= a.worker_id < a.num_workers, "--worker-id must lie in [0, --num-workers)"))


def _check_query(ap, a):
    filtered = any(x is not None for x in (a.only, a.only_file, a.exclude, a.exclude_file, a.within))
    clauses = [c.split("|") for c in a.sentences] if a.all_ else []
    _refuse(ap,
            (a.all_ and (a.moments or a.sequence or a.rerank or a.coarse is not None or a.width is not None or a.pool is not None),
             "--all does not go with --moments / --sequence / --rerank / --coarse"),
            (a.all_ and filtered, "--all does not go with --only / --exclude / --within"),
            (not a.all_ and (a.none is not None or a.veto is not None), "--none / --veto need --all"),
            (a.none is not None and a.veto is None, "--none needs --veto"),
            (a.veto is not None and a.none is None, "--veto needs --none"),
            (a.veto is not None and a.veto != a.veto, "--veto must not be NaN"),
            (any(not s.strip() for c in clauses for s in c), "--all: an empty alternative"),
            (sum(len(c) for c in clauses) + len(a.none or ()) > 32, "--all takes at most 32 sentences, alternatives and --none included"),
            (a.sequence and (a.moments or a.width is not None), "--sequence does not go with --moments / --width"),
            (a.sequence and len(a.sentences) > 32, "--sequence takes at most 32 sentences"),
            (a.rerank and (a.sequence or a.moments), "--rerank does not go with --sequence / --moments"),
            (a.rerank and (a.shard or a.host_resident), "--rerank does not go with --shard / --host-resident; merge the index files"),
            (a.pool is not None and not a.rerank and a.coarse is None, "--pool needs --rerank or --coarse"),
            (a.pool is not None and a.rerank and not 1 <= a.pool <= 32, "--pool must lie in [1, 32]"),
            (a.pool is not None and a.pool < 1, "--pool must be at least 1"),
            (a.coarse is not None and (a.sequence or a.moments or a.rerank), "--coarse does not go with --sequence / --moments / --rerank"),
            (a.coarse is not None and filtered, "--coarse does not go with --only / --exclude / --within"),
            (a.width is not None and not a.moments, "--width needs --moments"),
            (a.width is not None and not a.width >= 0, "--width must be >= 0"),
            (filtered and a.sequence, "--only / --exclude / --within do not go with --sequence"),
            (a.within is not None and a.rerank, "--within does not go with --rerank (the joint window is cut around the dual second)"))
    try:
        a.within = None if a.within is None else [parse_within(w) for w in a.within]
    except ValueError as e:
        ap.error(str(e))
    a.clauses = [[s.strip() for s in c] for c in clauses]


def _check_annotate(ap, a):
    smooth = a.smooth is not None
    _refuse(ap,
            ((a.labels is None) == (a.clusters is None), "one of --labels and --clusters is required"),
            (a.labels is not None and (a.checkpoint is None or a.vocab is None),
             "the following arguments are required: --checkpoint, --vocab"),
            (not 1 <= a.k <= 32, "-k must lie in [1, 32]"),
            (a.per_second and (a.threshold is not None or a.min_len is not None), "--per-second does not go with --threshold / --min-len"),
            (a.threshold is not None and a.threshold != a.threshold, "--threshold must not be NaN"),
            (a.min_len is not None and a.min_len < 1, "--min-len must be >= 1"),
            (smooth and a.per_second, "--smooth does not go with --per-second"),
            (smooth and not a.smooth >= 0, "--smooth must be >= 0"),
            (smooth and (a.threshold is None or not np.isfinite(a.threshold)), "--smooth needs a finite --threshold"))


def _check_discover(ap, a):
    smooth = a.smooth is not None
    _refuse(ap,
            (not 1 <= a.k <= MAX_CLUSTERS, f"-k must lie in [1, {MAX_CLUSTERS}]"),
            (a.iters < 1, "--iters must be >= 1"),
            (a.exemplars is not None and not 1 <= a.exemplars <= 32, "--exemplars must lie in [1, 32]"),
            (a.labels is not None and (a.checkpoint is None or a.vocab is None), "--labels needs --checkpoint and --vocab"),
            (a.labels is None and (a.checkpoint is not None or a.vocab is not None), "--checkpoint / --vocab need --labels"),
            (a.segments is None and any(x is not None for x in (a.threshold, a.min_len, a.smooth)),
             "--threshold / --min-len / --smooth need --segments"),
            (a.threshold is not None and a.threshold != a.threshold, "--threshold must not be NaN"),
            (a.min_len is not None and a.min_len < 1, "--min-len must be >= 1"),
            (smooth and not a.smooth >= 0, "--smooth must be >= 0"),
            (smooth and (a.threshold is None or not np.isfinite(a.threshold)), "--smooth needs a finite --threshold"))


def _check_similar(ap, a):
    _refuse(ap,
            (a.cover and a.align, "--cover does not go with --align"),
            (a.rank is not None and not a.cover, "--rank needs --cover"),
            (not a.align and any(x is not None for x in (a.threshold, a.skew, a.pool, a.piece)),
             "--threshold / --skew / --pool / --piece need --align"),
            (a.map is not None and not a.align, "--map needs --align"),
            (a.align and (a.threshold is None or not np.isfinite(a.threshold)), "--align needs a finite --threshold"),
            (a.align and a.skew is not None and not (a.skew >= 0 and np.isfinite(a.skew)), "--skew must be >= 0 and finite"),
            (a.align and a.pool is not None and not 1 <= a.pool <= 32, "--pool must lie in [1, 32]"),
            (a.align and a.piece is not None and not 1 <= a.piece <= MAX_CLIP_SECONDS, f"--piece must lie in [1, {MAX_CLIP_SECONDS}]"),
            (a.align and a.k < 1, "-k must be >= 1"),
            (not a.align and not 1 <= a.k <= (32 if a.keep_source else 31), "-k must lie in [1, 31], or [1, 32] with --keep-source"))
    try:
        a.clip = [parse_within(c, "--clip") for c in a.clip]
    except ValueError as e:
        ap.error(str(e))
    most = MAX_ALIGN_SECONDS if a.align else MAX_COVER_SECONDS if a.cover else MAX_CLIP_SECONDS
    for vid, first, last in a.clip:
        if first > last:
            ap.error(f"--clip {vid}:{first}-{last}: FIRST is after LAST")
        if last - first + 1 > most:
            ap.error(f"--clip {vid}:{first}-{last} holds {last - first + 1} seconds; cut it into clips of at most {most} seconds")


def _check_storyboard(ap, a):
    _refuse(ap,
            (not 1 <= a.k <= MAX_STORYBOARD_K, f"-k must lie in [1, {MAX_STORYBOARD_K}]"),
            (a.min_gain is not None and not (a.min_gain >= 0 and np.isfinite(a.min_gain)), "--min-gain must be >= 0 and finite"),
            (a.only is not None and a.only_file is not None, "--only does not go with --only-file"))


def _check_chapters(ap, a):
    _refuse(ap,
            (not 1 <= a.k <= MAX_CHAPTER_K, f"-k must lie in [1, {MAX_CHAPTER_K}]"),
            (not (a.penalty >= 0 and np.isfinite(a.penalty)), "--penalty must be >= 0 and finite"),
            (a.min_len is not None and not 1 <= a.min_len <= MAX_CHAPTER_SECONDS, f"--min-len must lie in [1, {MAX_CHAPTER_SECONDS}]"),
            (a.only is not None and a.only_file is not None, "--only does not go with --only-file"))


def parse_within(text, option="--within"):
    """'VID:FIRST-LAST' -> (vid, first, last); the vid may hold colons itself"""
    vid, sep, span = text.rpartition(":")
    first, dash, last = span.partition("-")
    if not sep or not vid or not dash or not first.isdigit() or not last.isdigit():
        raise ValueError(f"{option} takes VID:FIRST-LAST (seconds, inclusive), not {text!r}")
    return vid, int(first), int(last)


def _read_vids(path):
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def restrict_from_args(index, a):
    """The `RowFilter` of `query`'s --only / --only-file / --exclude / --exclude-file / --within, or None without any of them"""
    only = (a.only or []) + (_read_vids(a.only_file) if a.only_file else [])
    exclude = (a.exclude or []) + (_read_vids(a.exclude_file) if a.exclude_file else [])
    if not (only or exclude or a.within or a.only is not None or a.only_file):
        return None
    return index.restrict(videos=only if (a.only is not None or a.only_file) else None, exclude=exclude or None, windows=a.within)


def _load_index(a):
    """--index [--shard ...] [--host-resident] -> a `VideoIndex` or a `ShardedIndex`"""
    if a.shard or a.host_resident:
        return ShardedIndex.load([a.index] + (a.shard or []), resident="host" if a.host_resident else "device")
    return VideoIndex.load(a.index)


def _load_model(a):
    """(the aligner, its sentence embedder) of --checkpoint --vocab"""
    vocab = np.load(a.vocab)
    model = build_aligner(a.checkpoint, vocab, a.model, a.dtype)
    from ..word2vec_model import Word2VecTokenizer
    return model, make_embed_text(model, Word2VecTokenizer(max_words=32, vocab=vocab))


def _load_searcher(a):
    """(the aligner, its sentence embedder, the index) of `query` and `annotate`, loaded in this order"""
    return (*_load_model(a), _load_index(a))


def _run_merge(a):
    idx = VideoIndex.concat([VideoIndex.load(p, device="cpu") for p in a.inputs])
    idx.save(a.out)
    print(f"{a.out}: {len(idx)} seconds of {len(idx.vids)} videos from {len(a.inputs)} files", file=sys.stderr)
    return 0


def _run_coarse(a):
    idx = _load_index(a)
    image = CoarseImage.build(idx)
    image.save(a.out)
    print(f"{a.out}: {len(idx)} seconds in {len(image.parts)} shards, {image.nbytes()} bytes", file=sys.stderr)
    return 0


def _run_index(a):
    model = build_aligner(a.checkpoint, np.load(a.vocab), a.model, a.dtype)
    corpus = read_corpus(a.feature_dir, a.asr_json, a.vlen_csv, a.worker_id, a.num_workers)
    idx = build_index(model, corpus, dtype={"bf16": torch.bfloat16, "fp32": torch.float32, "e4m3": E4M3}[a.index_dtype or a.dtype],
                      keep_stem=a.keep_stem)
    idx.save(a.out)
    print(f"{a.out}: {len(idx)} seconds of {len(idx.vids)} videos", file=sys.stderr)
    return 0


def _run_similar(a):
    idx = _load_index(a)
    try:
        if a.align:
            found = search_copies(idx, a.clip, a.k, 32 if a.pool is None else a.pool, 16 if a.piece is None else a.piece,
                                  threshold=a.threshold, skew=a.skew or 0.0, exclude_source=not a.keep_source,
                                  paths=a.map is not None)
        elif a.cover:
            found = search_cover(idx, a.clip, a.k, a.rank or "both", exclude_source=not a.keep_source)
        else:
            found = search_clips(idx, a.clip, a.k, exclude_source=not a.keep_source)
    except ValueError as e:
        print(f"similar: {e}", file=sys.stderr)
        return 2
    if a.cover:
        for hits in found:
            for h in hits:
                print(f"{h.vid}\t{h.score:.6f}\t{h.forward:.6f}\t{h.backward:.6f}")
        return 0
    if a.map is not None:                              # only with --align
        with open(a.map, "w") as f:
            f.write("query,vid,query_second,first,last\n")
            for (vid, first, last), hits in zip(a.clip, found):
                for h, seconds in hits:
                    for i, (lo, hi) in enumerate(seconds.tolist()):
                        f.write(f"{vid}:{first}-{last},{h.vid},{first + h.q_start + i},{lo},{hi}\n")
        found = [[h for h, _ in hits] for hits in found]
    for hits in found:
        for h in hits:
            print(f"{h.vid}\t{h.start}\t{h.end}\t{h.score:.6f}" + (f"\t{h.q_start}\t{h.q_end}\t{h.cells}" if a.align else ""))
    return 0


def _run_storyboard(a):
    idx = _load_index(a)
    only = a.only if a.only is not None else _read_vids(a.only_file) if a.only_file is not None else None
    try:
        board = storyboard(idx, a.k, videos=only, min_gain=a.min_gain or 0.0, skip_long=a.skip_long)
    except (ValueError, KeyError) as e:
        print(f"storyboard: {e.args[0] if isinstance(e, KeyError) else e}", file=sys.stderr)
        return 2
    with open(a.out, "w", newline="") as f:
        write_storyboard_csv(f, board)
    if a.npz is not None:
        board.save(a.npz)
    print(f"{a.out}: {int((board.second >= 0).sum())} seconds of {len(board)} videos" +
          (f", {len(board.skipped)} over-long videos left out" if board.skipped else ""), file=sys.stderr)
    return 0


def _write_segments(path, ann, a):
    with open(path, "w", newline="") as f:
        write_segments_csv(f, ann.segments(float("-inf") if a.threshold is None else a.threshold, a.min_len or 1, switch=a.smooth))


def _run_discover(a):
    idx = _load_index(a)
    try:
        found = discover_steps(idx, a.k, a.iters, a.seed)
    except ValueError as e:
        print(f"discover: {e}", file=sys.stderr)
        return 2
    found.save(a.out)
    names = found.name(idx, *_load_model(a), _read_vids(a.labels)) if a.labels else None
    best = found.exemplars(idx, a.exemplars) if a.exemplars else None
    for c in range(len(found)):                        # cluster, seconds, cohesion[, name, its score][, vid:second:score ...]
        row = [str(c), str(int(found.sizes[c])), f"{found.cohesion[c]:.6f}"]
        if names is not None:
            row += [names[c][0], f"{names[c][1]:.6f}"]
        if best is not None:
            row += [f"{vid}:{sec}:{score:.6f}" for vid, sec, score in best[c]]
        print("\t".join(row))
    if a.segments is not None:
        k = 1 if a.smooth is None else min(5, len(found))                      # a decode chooses among a second's k best steps
        _write_segments(a.segments, found.annotation(idx, k, None if names is None else [n for n, _ in names]), a)
    print(f"{a.out}: {len(found)} steps over {len(idx)} seconds of {len(idx.vids)} videos, {len(found.moved)} passes, "
          f"{int((found.sizes == 0).sum())} empty", file=sys.stderr)
    return 0


def _run_annotate(a):
    if a.clusters is not None:
        idx = _load_index(a)
        found = StepClusters.load(a.clusters, idx.device)
        if a.k > len(found):
            print(f"annotate: -k {a.k} exceeds the {len(found)} steps of {a.clusters}", file=sys.stderr)
            return 2
        ann = found.annotation(idx, a.k)
    else:
        model, embed, idx = _load_searcher(a)
        ann = annotate(idx, model, embed, _read_vids(a.labels), a.k)
    with open(a.out, "w", newline="") as f:
        if a.per_second:
            write_per_second_csv(f, ann)
        else:
            write_segments_csv(f, ann.segments(float("-inf") if a.threshold is None else a.threshold, a.min_len or 1, switch=a.smooth))
    print(f"{a.out}: {len(ann)} seconds of {len(ann.vids)} videos against {len(ann.labels)} labels", file=sys.stderr)
    return 0


def _run_query(a):
    model, embed, idx = _load_searcher(a)
    only = restrict_from_args(idx, a)                  # None with --sequence, which takes no filter options
    if a.all_:
        for h in search_compound(idx, model, embed, [Compound(a.clauses, a.none or ())], a.k, veto=a.veto)[0]:
            print(f"{h.vid}\t{h.score:.6f}\t" + "\t".join(f"{t}:{p:.6f}" for t, p in zip(h.seconds, h.scores)))
    elif a.sequence:
        for h in search_sequences(idx, model, embed, [a.sentences], a.k)[0]:
            print(f"{h.vid}\t{h.score:.6f}\t" + "\t".join(str(t) for t in h.seconds))
    elif a.rerank:
        pool = 32 if a.pool is None else a.pool
        for sentence, hits in zip(a.sentences, search_rerank(idx, model, embed, a.sentences, min(a.k, pool), pool, restrict=only)):
            for h in hits:
                al = "" if h.alignability is None else f"{h.alignability:.6f}"
                print(f"{sentence}\t{h.vid}\t{h.second}\t{h.score:.6f}\t{h.confidence:.6f}\t{al}\t{h.dual_second}\t{h.dual_score:.6f}")
    elif a.moments:
        width = TEMPERATURE if a.width is None else a.width
        for sentence, hits in zip(a.sentences, search_moments(idx, model, embed, a.sentences, a.k, width, restrict=only)):
            for m in hits:
                print(f"{sentence}\t{m.vid}\t{m.start}\t{m.end}\t{m.second}\t{m.score:.6f}")
    else:
        image = None if a.coarse is None else CoarseImage.load(a.coarse, idx.device)
        if image is not None:
            try:
                image.check(idx)
            except ValueError as e:                    # an image of another index
                print(f"query: {e}", file=sys.stderr)
                return 2
        found = search(idx, model, embed, a.sentences, a.k, restrict=only, coarse=image, pool=64 if a.pool is None else a.pool)
        for sentence, hits in zip(a.sentences, found):
            for vid, sec, score in hits:
                print(f"{sentence}\t{vid}\t{sec}\t{score:.6f}")
    return 0


def _run_chapters(a):
    idx = _load_index(a)
    only = a.only if a.only is not None else _read_vids(a.only_file) if a.only_file is not None else None
    try:
        chaps = chapters(idx, a.k, penalty=a.penalty, min_len=a.min_len or 1, videos=only, skip_long=a.skip_long)
    except (ValueError, KeyError) as e:
        print(f"chapters: {e.args[0] if isinstance(e, KeyError) else e}", file=sys.stderr)
        return 2
    with open(a.out, "w", newline="") as f:
        write_chapters_csv(f, chaps)
    if a.npz is not None:
        chaps.save(a.npz)
    print(f"{a.out}: {int(chaps.count.sum())} chapters of {len(chaps)} videos" +
          (f", {len(chaps.skipped)} over-long videos left out" if chaps.skipped else ""), file=sys.stderr)
    return 0


_CHECKS = dict(index=_check_index, query=_check_query, annotate=_check_annotate, similar=_check_similar, discover=_check_discover,
               merge=lambda ap, a: None, coarse=lambda ap, a: None, storyboard=_check_storyboard, chapters=_check_chapters)
_RUNS = dict(index=_run_index, query=_run_query, annotate=_run_annotate, similar=_run_similar, discover=_run_discover, merge=_run_merge,
             coarse=_run_coarse, storyboard=_run_storyboard, chapters=_run_chapters)


def main(argv=None):
    a = parse_args(argv)
    return _RUNS[a.cmd](a)
