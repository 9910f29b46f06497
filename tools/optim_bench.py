#!/usr/bin/env python3
"""Time every fused clip + optimiser-step kernel (a2c_clip_*) on its own, RMSprop and Adam included as yardsticks.

Two sizes: n = 2^26 parameters (the state of the two-array rules, 1.5 GiB with params and grads, is far larger than the
256 MiB Infinity Cache, so every launch streams from HBM) and the trainable arena of the headline A3CModel (Pong, 3
actions), which is small enough to be launch-bound.  Bytes per launch = n * (16 + 8 * state arrays): params and grads
are read and written, and so is each state array.  GB/s = bytes / time; "of_peak" is that over 8 TB/s (HBM3E spec).

    python tools/optim_bench.py --out profiles/optim_bench.json                 # device-event timings
    rocprofv3 --kernel-trace --stats -d DIR -o optim -- python tools/optim_bench.py --iters 20 --warmup 5 --out ''
    python tools/optim_bench.py --merge-stats DIR/optim_results.db --out profiles/optim_bench.json

The event timings bracket `iters` back-to-back launches after `warmup` ones.  --merge-stats adds the kernel times of a
separate rocprofv3 run (its SQLite output, or the kernel_trace.csv of --output-format csv): the median dispatch
duration of each kernel at each size."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-a2c_amd")]

PEAK = 8.0e12
# name -> (state arrays, kernel-name key in a trace)
RULES = {"RMSprop": (1, "clip_rmsprop_kernel"), "Adam": (2, "clip_adam_kernel"), "SGD": (0, "SgdRule"),
         "Adagrad": (1, "AdagradRule"), "Adadelta": (2, "AdadeltaRule"), "Rprop": (2, "RpropRule"),
         "AdamW": (2, "AdamWRule"), "Adamax": (2, "AdamaxRule"), "NAdam": (2, "NAdamRule"), "RAdam": (2, "RAdamRule"),
         "ASGD": (1, "AsgdRule")}


def bytes_moved(name, n):
    return n * (16 + 8 * RULES[name][0])


def launcher(ops, name, p, g, s, sumsq, norm):
    step = [0]

    def run():
        step[0] += 1
        k = step[0]
        args = dict(RMSprop=lambda: ops.clip_rmsprop(p, g, s[0], sumsq, 1e30, 1e-4, 0.99, 1e-8, norm),
                    Adam=lambda: ops.clip_adam(p, g, s[0], s[1], sumsq, 1e30, 1e-4, 0.9, 0.999, 1e-8, k, norm),
                    SGD=lambda: ops.clip_sgd(p, g, sumsq, 1e30, 1e-4, norm),
                    Adagrad=lambda: ops.clip_adagrad(p, g, s[0], sumsq, 1e30, 1e-4, 0.0, 1e-10, k, norm),
                    Adadelta=lambda: ops.clip_adadelta(p, g, s[0], s[1], sumsq, 1e30, 1e-4, 0.9, 1e-6, norm),
                    Rprop=lambda: ops.clip_rprop(p, g, s[0], s[1], sumsq, 1e30, 0.5, 1.2, 1e-6, 50.0, norm),
                    AdamW=lambda: ops.clip_adamw(p, g, s[0], s[1], sumsq, 1e30, 1e-4, 0.9, 0.999, 1e-8, 0.01, k, norm),
                    Adamax=lambda: ops.clip_adamax(p, g, s[0], s[1], sumsq, 1e30, 1e-4, 0.9, 0.999, 1e-8, k, norm),
                    NAdam=lambda: ops.clip_nadam(p, g, s[0], s[1], sumsq, 1e30, 1e-4, 0.9, 0.999, 1e-8, 4e-3, k, 0.5,
                                                 norm),
                    RAdam=lambda: ops.clip_radam(p, g, s[0], s[1], sumsq, 1e30, 1e-4, 0.9, 0.999, 1e-8, k, norm),
                    ASGD=lambda: ops.clip_asgd(p, g, s[0], sumsq, 1e30, 1e-4, 1e-4, 0.5, norm))
        args[name]()
    return run


def headline_n_train():
    import a2c_amd
    net = a2c_amd.A3CModel([4, 84, 84], 3, h_size=256)
    net._ensure_device()
    return int(net._arena.n_train)


def measure(sizes, iters, warmup):
    import torch
    from a2c_amd import ops
    dev = "cuda"
    out = []
    for label, n in sizes:
        gen = torch.Generator(device=dev).manual_seed(0)
        p = torch.rand(n, device=dev, generator=gen) - 0.5
        g = (torch.rand(n, device=dev, generator=gen) - 0.5) * 1e-3
        s = [torch.zeros(n, device=dev) for _ in range(2)]
        sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        norm = torch.zeros(1, device=dev)
        ops.gradnorm_sq(g, sumsq)
        for name in RULES:
            for t in s:
                t.fill_(1e-3)          # Rprop's step sizes / Adagrad's sums start positive; the others do not care
            run = launcher(ops, name, p, g, s, sumsq, norm)
            for _ in range(warmup):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            sec = e0.elapsed_time(e1) / 1e3 / iters
            b = bytes_moved(name, n)
            out.append(dict(size=label, n=n, optimizer=name, state_arrays=RULES[name][0], bytes=b,
                            event_us=round(sec * 1e6, 2), event_GBps=round(b / sec / 1e9, 1),
                            event_of_peak=round(b / sec / PEAK, 3)))
            print(json.dumps(out[-1]), flush=True)
        del p, g, s
        torch.cuda.empty_cache()
    return out


def _trace_durations(path):
    """kernel name -> durations (ns) in dispatch order, from rocprofv3's output: its SQLite database (the default) or
    the kernel_trace.csv of --output-format csv"""
    out = {}
    if path.endswith(".db"):
        import sqlite3
        rows = sqlite3.connect(path).execute("select name, duration from kernels order by start")
    else:
        with open(path) as f:
            rows = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(f)]
    for kname, ns in rows:
        for name, (_, key) in RULES.items():
            if key in kname:
                out.setdefault(name, []).append(int(ns))
    return out


def merge_stats(rows, path):
    """add the kernel times of a separate rocprofv3 run of this tool: it launches each kernel the same number of times
    at each size, the big size first, so each kernel's dispatches split in two halves; the first quarter of each half
    (warm-up) is dropped and the median kept"""
    durs = _trace_durations(path)
    for row in rows:
        d = durs.get(row["optimizer"], [])
        half = len(d) // 2
        part = d[:half] if row["size"] == "2^26" else d[half:]
        part = part[len(part) // 4:]
        if part:
            ns = sorted(part)[len(part) // 2]
            row.update(kernel_us=round(ns / 1e3, 2), kernel_GBps=round(row["bytes"] / ns, 1),
                       kernel_of_peak=round(row["bytes"] / ns * 1e9 / PEAK, 3))
    for size in {r["size"] for r in rows}:
        ref = next((r for r in rows if r["size"] == size and r["optimizer"] == "Adam"), None)
        for r in rows:
            if r["size"] == size and ref is not None and "kernel_GBps" in r and "kernel_GBps" in ref:
                r["vs_adam_bandwidth"] = round(r["kernel_GBps"] / ref["kernel_GBps"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    ap.add_argument("--merge-stats", default=None, help="rocprofv3 output (.db, or kernel_trace.csv) of a separate run of this tool")
    a = ap.parse_args()
    if a.merge_stats:
        doc = json.load(open(a.out))
        doc["rows"] = merge_stats(doc["rows"], a.merge_stats)
        doc["kernel_times"] = ("median of rocprofv3 --kernel-trace durations, separate run (--iters 20 --warmup 5), "
                               "first quarter dropped")
    else:
        sizes = [("2^26", 1 << 26), ("a3c_n_train", headline_n_train())]
        doc = dict(tool="tools/optim_bench.py", peak_Bps=PEAK, bytes_per_param="16 + 8 * state arrays",
                   iters=a.iters, warmup=a.warmup, rows=measure(sizes, a.iters, a.warmup))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
