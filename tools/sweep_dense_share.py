"""Developer tool (GPU box): bench.py under another dense share.  AOC_DENSE_SHARE = the share in 256ths (1 .. 256) of the stream's CUs
that dense_prune_kernel's resident workgroups take (aoc_set_dense_share); unset = the library's default.  Everything else is bench.py's:
the arguments are passed through and the result line is the bench's own, so a sweep is one run of this file per share, alternating with
the share one compares against.
Usage: AOC_DENSE_SHARE=192 python tools/sweep_dense_share.py --gpus 1 --steps 20 --warmup 5"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

aoc = importlib.import_module("robust-video-object-segmentation_amd")
share = os.environ.get("AOC_DENSE_SHARE", "")
now = aoc.ops.set_stream_cus(dense_share=int(share) if share else None)
print(f"sweep_dense_share: share {now}/256", file=sys.stderr)
bench.main()
