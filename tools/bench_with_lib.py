"""bench.py against another build of the library: python tools/bench_with_lib.py <libdae_hip.so> [bench.py arguments]."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dae_rnn_news_recommendation_amd import _lib as L

L.LIB_PATH = L.LIB_PATHS["bf16"] = os.path.abspath(sys.argv[1])      # _lib.load reads LIB_PATHS
sys.argv = ["bench.py"] + sys.argv[2:]
import bench

bench.main()
