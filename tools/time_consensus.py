"""Device time of povu_hip_vcf_consensus (HipDecomposer.consensus) on a synthetic cohort: one reference path of --length bases
(a chain of 4 KiB segments, every third walked backwards), --samples haploid sample columns, a record every --every bases
(SNVs, short insertions and deletions in turn; every sample carries about half of them).  The text stays on the device
(text=False), so the call's time holds no copy of the output to the host.

The yardstick is not the code under test: a device-to-device hipMemcpyAsync of the same byte count in the same process, on the
same box, timed by HIP events.  One JSON line per run -- the call's HIP-event time, the materialiser's own (write_ms), the
bytes it wrote and their rate, the copy's rate -- then a line with the medians of the runs behind the warm-up runs.  No
threshold is set.

    python tools/time_consensus.py [--samples 64] [--length 16777216] [--every 1000] [--warmup 2] [--runs 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEGMENT = 4096


def chain(length: int, rng):
    """(links, paths, sequences, bases) of one path `ref` that spells `length` random bases."""
    from povu_amd import workloads as W
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=length)
    n = (length + SEGMENT - 1) // SEGMENT
    rev = (np.arange(n) % 3 == 1).astype(np.int64)
    seqs = []
    for k in range(n):
        piece = text[k * SEGMENT:(k + 1) * SEGMENT]
        seqs.append((comp[piece][::-1] if rev[k] else piece).tobytes().decode())
    ids = np.arange(1, n + 1)
    v1, v2 = np.arange(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64)
    s1 = np.where(rev[:-1] == 1, W.L, W.R).astype(np.int64)
    s2 = np.where(rev[1:] == 1, W.R, W.L).astype(np.int64)
    links = W._mk(ids, v1, s1, v2, s2)
    return links, W._paths(["ref"], [(ids.tolist(), rev.tolist())]), seqs, text.tobytes().decode()


def cohort_vcf(bases: str, samples: int, every: int, rng) -> str:
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"s{k}" for k in range(samples)) + "\n"
    out = [head]
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    for k, at in enumerate(range(every, len(bases) - 16, every)):
        ref = bases[at]
        if k % 3 == 0:
            r, a = ref, other[ref]
        elif k % 3 == 1:
            r, a = ref, ref + "acgtacgt"[:1 + k % 8]
        else:
            r, a = bases[at:at + 2 + k % 7], ref
        gts = "\t".join(rng.choice(["0", "1"], size=samples))
        out.append(f"ref\t{at + 1}\tv{k}\t{r}\t{a}\t60\tPASS\t.\tGT\t{gts}\n")
    return "".join(out)


def copy_rate(n_bytes: int, runs: int) -> float:
    """Bytes per second of a device-to-device hipMemcpyAsync of n_bytes on the null stream, by HIP events (the median of `runs`,
    one warm-up before): the runtime the library is linked against, called directly."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: HIP error {rc}")

    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes)), "hipMalloc")
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)), "hipMalloc")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    ok(hip.hipMemsetAsync(src, 65, n_bytes, None), "hipMemsetAsync")
    times = []
    for k in range(runs + 1):
        ok(hip.hipEventRecord(e0, None), "hipEventRecord")
        ok(hip.hipMemcpyAsync(dst, src, n_bytes, 3, None), "hipMemcpyAsync")  # 3: hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float(0)
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        if k:
            times.append(ms.value)
    for p in (src, dst):
        hip.hipFree(p)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    return n_bytes / (statistics.median(times) * 1e-3)


def main():
    from povu_amd import HipDecomposer
    from povu_amd import hip as H
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--length", type=int, default=1 << 24)
    ap.add_argument("--every", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    links, paths, seqs, bases = chain(a.length, rng)
    doc = H.parse_vcf(cohort_vcf(bases, a.samples, a.every, rng), threads=16)
    d = HipDecomposer(0)
    d.upload(links)
    d.upload_paths(paths)
    d.upload_sequences(seqs)
    rows = []
    for k in range(a.warmup + a.runs):
        c = d.consensus(doc, text=False, time_write=True)
        row = dict(run=k, samples=a.samples, length=a.length, records=doc.n_records, haplotypes=c.n_haps, applied=int(c.n_applied.sum()),
                   bytes=c.n_text_bytes, device_ms=round(c.device_ms, 3), write_ms=round(c.write_ms, 4),
                   write_GBps=round(c.n_text_bytes / (c.write_ms * 1e-3) / 1e9, 1) if c.write_ms else None)
        print(json.dumps(row), flush=True)
        if k >= a.warmup:
            rows.append(row)
    n = rows[0]["bytes"]
    copy = copy_rate(n, a.runs)
    d.close()
    write_ms = statistics.median(r["write_ms"] for r in rows)
    print(json.dumps(dict(median=True, bytes=n, device_ms=statistics.median(r["device_ms"] for r in rows), write_ms=write_ms,
                          write_GBps=round(n / (write_ms * 1e-3) / 1e9, 1), copy_d2d_GBps=round(copy / 1e9, 1))))


if __name__ == "__main__":
    main()
