#!/usr/bin/env python3
"""Times msw_sort_pairs_device and msw_markdup_device on the GPU.

Sort: n uniformly random u64 keys with an iota u32 value array, HBM-resident,
timed with device events on torch's current stream, beside
torch.sort(stable=True) on the same keys on the same device.  Like for like:
both return the sorted keys AND the permutation (torch's int64 indices are its
value array); torch is given the keys already masked to key_bits, since it has
no key_bits of its own; the copy that restores the unsorted keys before each
in-place sort is outside the timed window.  The two alternate, repetition by
repetition.  np.argsort(kind="stable") runs on the host for the smaller sizes
(numpy sorts on one thread, however many CPUs there are).

Duplicates: msw_markdup_device on synthetic 150-base records (one M op, one in
ten behind a 5-base clip) spread uniformly over a 4 Mbase genome, single-end
and as pairs (one pair in ten repeats the pair before it).

One JSON line per measurement, on stdout and in --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_parallel_amd as mpa  # noqa: E402


def timed(fn, before=None):
    if before:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3)}


def bench_sort(ctx, n, key_bits, reps, host, emit):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(n + key_bits)
    keys = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device="cuda", generator=gen)
    mask = (1 << key_bits) - 1
    masked = keys & (mask if key_bits < 64 else -1)
    work, vals = torch.empty_like(keys), torch.empty(n, dtype=torch.int32, device="cuda")
    iota = torch.arange(n, dtype=torch.int32, device="cuda")

    def reset():
        work.copy_(keys)
        vals.copy_(iota)

    ours = lambda: ctx.sort_pairs_device(work.data_ptr(), vals.data_ptr(), n, key_bits, stream=stream)
    theirs = lambda: torch.sort(masked, stable=True)
    timed(ours, reset)
    _, (tv, ti) = timed(theirs)
    # the same keys in the same order; below 64 bits torch saw the same unsigned order, so the same permutation
    if key_bits < 64:
        assert bool(((work & mask) == tv).all()) and bool((vals.long() == ti).all())
    else:
        u = work ^ (-2 ** 63)
        assert bool((u[1:] >= u[:-1]).all())
    assert bool((keys[vals.long()] == work).all())
    del tv, ti
    t_ours, t_torch = [], []
    for _ in range(reps):
        t_ours.append(timed(ours, reset)[0])
        t_torch.append(timed(theirs)[0])
    passes = (key_bits + 7) // 8
    # a pass reads the keys for the histogram, reads keys and values again and writes both: 8 + 12 + 12 bytes an
    # element; an odd pass count adds the copy back, 12 + 12
    traffic = n * (32 * passes + (24 if passes % 2 else 0))
    rec = {"what": "sort", "n": n, "key_bits": key_bits, "passes": passes, "ours": spread(t_ours),
           "torch_sort_stable": spread(t_torch), "ours_gbps_of_traffic": round(traffic / min(t_ours) / 1e6, 1),
           "speedup_median": round(float(np.median(t_torch) / np.median(t_ours)), 2)}
    if host:
        hk = masked.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        np.argsort(hk, kind="stable")
        rec["numpy_argsort_stable_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    emit(rec)


def bench_markdup(ctx, n, pairs, reps, emit):
    stream = torch.cuda.current_stream().cuda_stream
    ref_len = 4 << 20
    gen = torch.Generator(device="cuda").manual_seed(n)
    clip = torch.rand(n, device="cuda", generator=gen) < 0.1
    ref_pos = torch.randint(0, ref_len - 150, (n,), dtype=torch.int64, device="cuda", generator=gen)
    strand = torch.randint(0, 2, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    score = torch.randint(200, 301, (n,), dtype=torch.int32, device="cuda", generator=gen)
    if pairs:  # two random pairs never share both keys: one pair in ten repeats the pair before it
        again = torch.nonzero(torch.rand(n // 2, device="cuda", generator=gen) < 0.1).flatten().clamp(min=1)
        for a in (clip, ref_pos, strand):
            a.view(n // 2, 2)[again] = a.view(n // 2, 2)[again - 1]
    nm = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    off[1:] = torch.cumsum(1 + clip.int(), 0)
    total = int(off[n])
    cig = torch.full((total + 1,), 150 << 4, dtype=torch.int32, device="cuda")
    first = off[:-1].long()
    cig[first[clip]] = 5 << 4 | 4
    cig[first[clip] + 1] = 145 << 4
    frags = n // 2 if pairs else n
    order = torch.empty(frags, dtype=torch.int32, device="cuda")
    dup = torch.empty(n, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    run = lambda: ctx.mark_duplicates_device(ref_pos.data_ptr(), nm.data_ptr(), off.data_ptr(), cig.data_ptr(), total,
                                             strand.data_ptr(), score.data_ptr(), n, ref_len, order.data_ptr(),
                                             dup.data_ptr(), cnt.data_ptr(), pairs=pairs, stream=stream)
    timed(run)
    ms = [timed(run)[0] for _ in range(reps)]
    assert int(dup.sum()) >= int(cnt[0]) > 0
    emit({"what": "markdup", "rows": n, "pairs": bool(pairs), "dup_fragments": int(cnt[0]), **spread(ms),
          "rows_per_s": round(n / min(ms) * 1e3)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 1 << 24, 1 << 27])
    ap.add_argument("--key-bits", type=int, nargs="+", default=[24, 32, 64])
    ap.add_argument("--markdup-rows", type=int, nargs="*", default=[800_000, 1 << 24])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=1 << 24, help="largest n np.argsort is timed at")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not mpa.is_gpu_available():
        sys.exit("sort_bench: no GPU (there is nothing to measure without one)")
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    ctx = mpa.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())  # a stream of its own: the library takes 0 for its own compute stream
    try:
        for n in a.sizes:
            for bits in a.key_bits:
                bench_sort(ctx, n, bits, a.reps, n <= a.host_max and bits == 64, emit)
        for n in a.markdup_rows:
            for pairs in (False, True):
                bench_markdup(ctx, n, pairs, a.reps, emit)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
