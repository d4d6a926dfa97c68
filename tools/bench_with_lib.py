"""bench.py against another build of the library: python tools/bench_with_lib.py <lib> [bench.py arguments].

<lib> is a directory that holds both builds (libdae_hip.so and libdae_hip_f16.so: the default precisions run on the fp16 build),
or one libdae_hip.so, which replaces the bf16 build only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dae_rnn_news_recommendation_amd import _lib as L

lib = os.path.abspath(sys.argv[1])
if os.path.isdir(lib):                                                # _lib.load reads LIB_PATHS
    for fmt, path in list(L.LIB_PATHS.items()):
        L.LIB_PATHS[fmt] = os.path.join(lib, os.path.basename(path))
    missing = [path for path in L.LIB_PATHS.values() if not os.path.isfile(path)]
    if missing:
        sys.exit("bench_with_lib: not found: " + ", ".join(missing))
    L.LIB_PATH = L.LIB_PATHS["bf16"]
else:
    L.LIB_PATH = L.LIB_PATHS["bf16"] = lib
sys.argv = ["bench.py"] + sys.argv[2:]
import bench

bench.main()
