"""What the channel family's bench tools (bench_ddc, bench_pfb, bench_bank, bench_resample, bench_welch) share: the host clock around a
call, the context's per-kernel events of a call, and the line a list of regions prints as."""
import statistics
import time

import torch


def stats(v):
    return f"{min(v):.3f} - {max(v):.3f} ms (median {statistics.median(v):.3f}, {len(v)} regions)"


def timed(e, fn):
    """Host clock around fn() + synchronise -> ms."""
    e.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    e.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernels(e, fn):
    """The kernels of fn() by the context's per-kernel events -> {name: ms}."""
    e.enable_timing(True)
    e.kernel_times()
    fn()
    e.sync()
    kt = e.kernel_times()
    e.enable_timing(False)
    return {k: sum(v) for k, v in kt.items()}
