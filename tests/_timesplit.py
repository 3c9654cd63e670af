"""What the time-split tests share (test_time_split_plan.py, test_time_split_batch_plan.py,
test_gpu_time_split*.py): the planner's lattice and default warmup, restated."""
import math


def _lattice(cfg):
    half = cfg.samplebuf_size // 2
    return half * 4 // math.gcd(half, 4)


def _default_warmup(cfg):
    return max(int(10.0 * cfg.sample_rate), 2 * cfg.samplebuf_size)
