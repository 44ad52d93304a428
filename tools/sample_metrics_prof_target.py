"""Profiling target for profiles/sample_metrics_cost.txt part (b): the symmetric squared-distance matrix at M = 512 (4 calls) and
M = 2048 (3 calls) rows of 32*128*128 voxels, N(0,1) data.  Run under rocprofv3 (see tools/sample_metrics_cost.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from saragan_amd.metrics import sample_metrics as SM                     # noqa: E402

V = 32 * 128 * 128
for M, reps in ((512, 4), (2048, 3)):
    g = torch.Generator(device='cuda').manual_seed(3)
    Z = torch.randn((M, V), device='cuda', generator=g)
    for _ in range(reps):
        SM.pairwise_sqdist(Z)
    torch.cuda.synchronize()
    del Z
    torch.cuda.empty_cache()
