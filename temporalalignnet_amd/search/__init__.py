"""Corpus search with the dual encoder: "which seconds of which videos match this sentence".

The reference's `get_visual_feature` "can be used for retrieval setting" (model/tan_model.py:152); `infer_align.align_corpus` asks
the dual encoder only about a video's own ASR sentences.  Here the video side is computed ONCE into a per-second index and any
sentence is ranked against all of it.  One module per concern -- `index`, `text` (with what every search shares), `video`,
`annotation`, `cluster`, `summary`, `cli` -- each with its own account of what it does; every public name is re-exported here, and only here.
A search starts from a sentence (`search`, `search_moments`, `search_sequences`, `search_compound`, `search_rerank`), from a vocabulary (`annotate`),
from a piece of video (`search_clips`, `search_copies`, `align_paths`, `search_cover`) -- or from nothing: `discover_steps` clusters the index's
seconds into the steps that recur in it, and its `StepClusters` serve as the vocabulary nobody had to write.  `storyboard` says what
a video looks like: the k seconds that together cover it best; `chapters` says where its parts begin and end.

    python -m temporalalignnet_amd.search index --checkpoint C --feature-dir F --asr-json A --vlen-csv V --vocab s3d_dict.npy --out I.npz
    python -m temporalalignnet_amd.search query --checkpoint C --vocab s3d_dict.npy --index I.npz -k 10 "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --moments [--width 0.07] "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --sequence "crack two eggs" "whisk them" "pour into the pan"
    python -m temporalalignnet_amd.search query ... --all "whisk eggs" "fry bacon|cook bacon" [--none "microwave" --veto 0.3] [-k K]
    python -m temporalalignnet_amd.search index ... --keep-stem;  ... query ... --rerank [--pool 32] "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --index I0.npz --shard I1.npz --shard I2.npz [--host-resident] "crack two eggs" ...
    python -m temporalalignnet_amd.search query ... --only VID --only-file vids.txt --exclude VID --within VID:30-90 "crack two eggs" ...
    python -m temporalalignnet_amd.search merge --out I.npz I0.npz I1.npz ...
    python -m temporalalignnet_amd.search coarse --index I.npz [--shard I1.npz ...] [--host-resident] --out I.c4.npz
    python -m temporalalignnet_amd.search query ... --index I.npz [--shard ...] [--host-resident] --coarse I.c4.npz [--pool 64] "crack two eggs" ...
    python -m temporalalignnet_amd.search annotate --checkpoint C --vocab s3d_dict.npy --index I.npz --labels steps.txt [-k K]
        [--threshold X] [--min-len M] [--smooth PENALTY] [--per-second] --out segments.csv
    python -m temporalalignnet_amd.search similar --index I.npz [--shard I1.npz ...] [--host-resident] --clip VID:10-29 [-k K] [--keep-source]
    python -m temporalalignnet_amd.search similar --index I.npz --clip VID:0-599 --align --threshold X [--skew Y] [--pool P] [--piece S] [-k K]
    python -m temporalalignnet_amd.search similar --index I.npz --clip VID:0-599 --align --threshold X --map OUT.csv
    python -m temporalalignnet_amd.search similar --index I.npz --clip VID:0-599 --cover [--rank both|query|video] [-k K] [--keep-source]
    python -m temporalalignnet_amd.search discover --index I.npz [--shard I1.npz ...] [--host-resident] -k 64 [--iters 10] [--seed 0]
        --out clusters.npz [--exemplars 3] [--labels steps.txt --checkpoint C --vocab V] [--segments seg.csv --threshold X [--min-len M] [--smooth P]]
    python -m temporalalignnet_amd.search annotate --index J.npz --clusters clusters.npz [-k K] [--threshold X] ... --out segments.csv
    python -m temporalalignnet_amd.search storyboard --index I.npz [--shard I1.npz ...] [--host-resident] [-k 8] [--min-gain X]
        [--only VID ... | --only-file F] [--skip-long] --out story.csv [--npz story.npz]
    python -m temporalalignnet_amd.search chapters --index I.npz [--shard I1.npz ...] [--host-resident] [-k 12] --penalty X [--min-len M]
        [--only VID ... | --only-file F] [--skip-long] --out chapters.csv [--npz chapters.npz]
"""
from .annotation import Annotation, annotate, label_lists, write_per_second_csv, write_segments_csv  # noqa: F401
from .cli import main, parse_args, parse_within, restrict_from_args                                 # noqa: F401
from .coarse import CoarseImage                                                                     # noqa: F401
from .cluster import MAX_CLUSTERS, StepClusters, centroid_image, discover_steps                      # noqa: F401
from .index import E4M3, RowFilter, ShardedIndex, VideoIndex, _index_chunks, build_index, plan_index_windows, restrict_spans  # noqa: F401
from .summary import (MAX_CHAPTER_K, MAX_CHAPTER_SECONDS, MAX_STORYBOARD_K, MAX_STORYBOARD_SECONDS, Chapters,  # noqa: F401
                      Storyboard, chapters, plan_passes, storyboard, write_chapters_csv, write_storyboard_csv)
from .text import (RERANK_TEXT_SLOTS, TEMPERATURE, Compound, CompoundHit, Moment, Reranked, SequenceHit, _rerank_table,  # noqa: F401
                   _Sweep, _TopLists, compound_tables, compound_weakest, query_features, rerank_window, search, search_compound,
                   search_moments, search_rerank, search_sequences)
from .video import (EMPTY_ROW, MAX_ALIGN_SECONDS, MAX_CLIP_SECONDS, MAX_COVER_SECONDS, PIECE_ROWS, ClipHit, CopyHit,  # noqa: F401
                    CopyPath, CoverHit, align_paths, align_spans, align_tables, clip_features, clip_spans, copy_interval,
                    copy_inverse, copy_pieces, drop_source, path_tables, piece_offsets, search_clips, search_copies, search_cover,
                    transfer_segments)
