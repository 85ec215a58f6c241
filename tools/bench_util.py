"""What the stage benchmarks (tools/*_bench.py) share: the timing of one call
and the result line."""
import json
import os


def timed(fn, reps):
    """Device events around each of ``reps`` calls of ``fn`` after a warm-up
    call (code object load, first touch, allocator, FFT plan): the median, the
    minimum and the maximum in ms."""
    import torch
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def emit(res, out=None):
    """Print ``res`` as one JSON line; with ``out`` write it to that file too."""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def timed_alternating(fns, reps):
    """``timed`` for several calls measured in turn: after one warm-up call of
    each, ``reps`` rounds that time every entry of the dict ``fns`` once, so a
    drift of the clocks meets all of them alike.  Returns {name: timed's dict}."""
    import torch
    for fn in fns.values():
        fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    return out
