#!/usr/bin/env python3
"""bench.py with its arguments, followed by one JSON line with the process's
peak device memory (torch allocator: allocated and reserved).

    python profiles/bench_peak_memory.py --gpus 1 --steps 20 --warmup 5
"""
import json
import os
import runpy
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.argv = ["bench.py"] + sys.argv[1:]
try:
    runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
finally:
    print(json.dumps({
        "peak_alloc_GB": torch.cuda.max_memory_allocated() / 1e9,
        "peak_reserved_GB": torch.cuda.max_memory_reserved() / 1e9}))
