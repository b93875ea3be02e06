"""The timing helpers of the bench tools (whisper_encoder_bench, whisper_decoder_bench, mel_bench):
an arm is the median of its repetitions, with the min and max a difference has to exceed."""
import statistics
import time


def summary(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "repeat": len(times)}


def timed(fn, repeat, warmup, sync=None):
    """Wall time of fn() (and sync(), for device work), per repetition."""
    sync = sync or (lambda: None)
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return summary(out)


def event_timed(fn, repeat, warmup, steps, torch):
    """Time per launch between device events around `steps` launches; fn(i): launch number i of
    a repetition."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / steps)
    s = summary(times)
    s["steps"] = steps
    return s


def beats(a, b):
    return {"speedup_median": b["median_s"] / a["median_s"], "not_slower_median": bool(a["median_s"] <= b["median_s"]),
            "beats_beyond_spread": bool(a["max_s"] < b["min_s"])}
