#!/usr/bin/env python3
"""GPU BGZF deflate throughput on FASTQ text resident in HBM: GB/s of input
for msw_bgzf_deflate_device (HIP events around >= 300 ms of launches, several
rounds, min-max), beside zlib level 1 over the same 65,280-byte blocks on the
CPUs and the GPU inflate of the result (MSW_GZ_TIMING prints its kernel times).
  python tools/deflate_bench.py --qual binned --mib 256"""
import argparse
import ctypes
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 0xFF00


def _z1(chunk):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return len(c.compress(chunk) + c.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qual", default="binned", choices=["binned", "illumina"])
    ap.add_argument("--mib", type=int, default=256, help="input bytes resident on the device")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpus", type=int, default=16)
    args = ap.parse_args()
    os.environ["MSW_GZ_TIMING"] = "1"
    import numpy as np
    import torch
    from mini_parallel_amd import Context, bgzf_inflate
    from mini_parallel_amd import synthetic as syn
    from mini_parallel_amd._lib import check, lib
    g = syn.wgs_genome()
    b, pos, rng = syn._lane_reads(g, 0, 20_000, 150, 2.0, 1004)
    text = syn._lane_records(b, pos, rng, b"SYN", 1, args.qual)
    n = args.mib << 20
    data = (text * (n // len(text) + 1))[:n]
    ctx = Context(0)
    L = lib()
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = L.msw_bgzf_deflate_bound(n)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream()

    def launch():
        check(L.msw_bgzf_deflate_device(ctx.handle, src.data_ptr(), n, out.data_ptr(), cap, out_len.data_ptr(), 0,
                                        ctypes.c_void_p(st.cuda_stream)))

    launch()
    torch.cuda.synchronize()
    clen = int(out_len.item())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch()
    e0.record(st)
    launch()
    e1.record(st)
    torch.cuda.synchronize()
    reps = max(1, int(300.0 / e0.elapsed_time(e1)) + 1)  # >= 300 ms between the events
    rates = []
    for _ in range(args.rounds):
        e0.record(st)
        for _ in range(reps):
            launch()
        e1.record(st)
        torch.cuda.synchronize()
        rates.append(n * reps / (e0.elapsed_time(e1) * 1e6))
    print(f"gpu deflate ({args.qual}): {n >> 20} MiB -> {clen} B (ratio {n / clen:.3f}), {reps} launches per round, "
          f"{min(rates):.2f}-{max(rates):.2f} GB/s of input", flush=True)
    blob = out[:clen].cpu().numpy().tobytes()
    chunks = [data[k:k + BLOCK] for k in range(0, n, BLOCK)]
    with ThreadPoolExecutor(args.cpus) as ex:  # zlib releases the GIL
        t = time.perf_counter()
        z = sum(ex.map(_z1, chunks, chunksize=64))
        dt = time.perf_counter() - t
    print(f"zlib level 1, {args.cpus} threads: {z} B payload, {n / dt / 1e9:.3f} GB/s; gpu bytes / zlib bytes = "
          f"{(clen - 26 * len(chunks) - 28) / z:.4f}", flush=True)
    assert bgzf_inflate(ctx, blob) == data  # MSW_GZ_TIMING: the inflate and CRC kernel times on stderr
    ctx.close()


if __name__ == "__main__":
    main()
