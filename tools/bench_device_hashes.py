#!/usr/bin/env python3
"""tools/bench_device_hashes.py -- the two device hash families on the same windows: SHA-1 (sha1_windows_kernel) as the baseline,
XXH32 and XXH64 (xxh_windows_kernel) next to it, every figure from the same run on the same box.

Corpus: that of tools/bench_device_shingles.py (seeded, synthetic, nothing downloaded).

  (a) kernels alone   the 5.0e7 windows of the shingles bench -- the first 50 000 documents, byte mode k = 5 and 9, token mode
               w = 3 -- through mhx_hash_windows with MHX_HASH_SHA1 / MHX_HASH_XXH at 32 bits and MHX_HASH_XXH at 64.  The
               MHX_API_XXH family has host forms only, so a call is upload + one kernel + download and the library offers no
               way to bracket the kernel with events; the kernel's own time comes from the device's dispatch timestamps
               instead: this part runs as a child under `rocprofv3 --kernel-trace` and the parent reads the trace.  Behind
               tools/_warm.py's clock warm-up (resident launches of mhx_sha1_windows_dev) the three kernels alternate, 11
               calls each, every call behind 8 untimed resident launches that keep the clocks up across the copies; all 11
               durations are printed.  The SHA-1 kernel timed here is the unchanged kernel: the baseline of this run.
  (b) end to end   host arrays in, results out, wall clock, the upload and the download included, three runs each of
               sha1_hash32, xxh32_hash32, xxh64_hash64 on the 200 000-document corpus: MinHash.bulk_signatures(documents=,
               shingle=9, num_perm=128) and HyperLogLog.bulk_registers(documents=, shingle=9, p=8) -- the registers at the width of
               the function, hash_bits=32 for sha1_hash32 and xxh32_hash32 and hash_bits=64 for xxh64_hash64 (the only pairing
               that reaches the device), so the third figure is the 64-bit register kernel, not a like-for-like of the first two.  PCIe carries 200 MB up
               and the results down in every one of them; no threshold is attached.  Runs as a child of its own, untraced.

`python tools/bench_device_hashes.py [--out profiles/hashes_bench.txt] [--work build/hashes_bench]`; the parent opens no device,
the two children run one after the other, each under a time limit.  SCALE (env, float, default 1) scales the document counts for
a dry run.  VALU_COUNTS below are read off the gfx950 listing (hipcc --offload-device-only -S, lines starting with v_) and are
what the predicted ratio is derived from."""
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402
from tools.bench_device_shingles import corpus, n_of  # noqa: E402

REPS = 11
PREROLL = 8
LIMIT = 600  # seconds per child
# static VALU instructions of the instantiations that hash byte shingles of 5 and 9 bytes (the gfx950 listing)
VALU_COUNTS = {"sha1_32": 901, "xxh_32": 233, "xxh_64": 417}
KERNELS = (("sha1_32", 0, 32), ("xxh_32", 1, 32), ("xxh_64", 1, 64))  # label, hash_kind, bits


def kernel_child(work):
    """Under rocprofv3: the calls, and work/sequence.json -- one label per *_windows_kernel dispatch, in launch order."""
    from datasketch_amd import _native, shingle
    from datasketch_amd._native import MHX_U32

    ctx = _native.context()
    text, doc_offsets, word_offsets, doc_words = corpus(n_of(50_000))
    d_text = ctx.to_device(text)
    sequence, shapes = [], []
    for mode, width in (("bytes", 5), ("bytes", 9), ("tokens", 3)):
        items, docs = (None, doc_offsets) if mode == "bytes" else (word_offsets, doc_words)
        set_offsets = shingle.window_offsets(docs, width)
        n_docs, n_windows = docs.size - 1, int(set_offsets[-1])
        d_items = None if items is None else ctx.to_device(items)
        d_docs, d_sets, d_out = ctx.to_device(docs), ctx.to_device(set_offsets), ctx.alloc(4 * n_windows)

        def resident():
            ctx.sha1_windows_dev(d_text.ptr, None if d_items is None else d_items.ptr, d_docs.ptr, d_sets.ptr, n_docs, n_windows, width, MHX_U32, d_out.ptr)

        for label, kind, bits in KERNELS:  # code objects, scratch
            ctx.hash_windows(text, docs, width, items, bits, kind)
            sequence.append("untimed")
        sequence += ["untimed"] * warm(resident, ctx.synchronize)
        for _ in range(REPS):
            for label, kind, bits in KERNELS:
                for _ in range(PREROLL):
                    resident()
                sequence += ["untimed"] * PREROLL
                ctx.hash_windows(text, docs, width, items, bits, kind)
                sequence.append(f"{mode}/{width}/{label}")
        shapes.append(dict(mode=mode, width=width, documents=int(n_docs), windows=n_windows, text_bytes=int(text.size)))
        for buf in (d_items, d_docs, d_sets, d_out):
            if buf is not None:
                buf.free()
    info = ctx.info()
    with open(os.path.join(work, "sequence.json"), "w") as f:
        json.dump(dict(sequence=sequence, shapes=shapes, device=info["name"], cus=info["compute_units"], library=os.path.basename(_native.LIB_PATH)), f)


def end_to_end_child(work):
    from datasketch_amd import HyperLogLog, MinHash, _native, sha1_hash32, xxh32_hash32, xxh64_hash64

    if not _native.gpu_available():
        raise SystemExit("bench_device_hashes.py needs an MI355X")
    text, doc_offsets, _, _ = corpus(n_of(200_000))
    n_docs = doc_offsets.size - 1
    small = (text[: int(doc_offsets[64])], doc_offsets[:65])
    lines = []
    for name, call in (("MinHash.bulk_signatures(shingle=9, num_perm=128)",
                        lambda docs, f: MinHash.bulk_signatures(documents=docs, shingle=9, num_perm=128, seed=1, hashfunc=f, out_dtype=np.uint32, gpu_mode="always")),
                       ("HyperLogLog.bulk_registers(shingle=9, p=8)",
                        lambda docs, f: HyperLogLog.bulk_registers(documents=docs, shingle=9, p=8, hashfunc=f, hash_bits=64 if f is xxh64_hash64 else 32,
                                                                   gpu_mode="always"))):
        rec = dict(what="(b) host in, results out", call=name, documents=int(n_docs), text_bytes=int(text.size))
        for f in (sha1_hash32, xxh32_hash32, xxh64_hash64):
            call(small, f)  # code objects
            call((text, doc_offsets), f)  # scratch at its final size
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                call((text, doc_offsets), f)
                runs.append(round(time.perf_counter() - t0, 4))
            rec[f.__name__ + "_seconds"] = runs
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    with open(os.path.join(work, "end_to_end.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def read_trace(work):
    """Durations (ms) of every *_windows_kernel dispatch of the child, in the order they started."""
    rows = []
    for path in glob.glob(os.path.join(work, "trace", "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "windows_kernel" in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    return [((end - start) / 1e6, name) for start, end, name in rows]


def kernels_alone(work, lines):
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(work, "trace"), "--", sys.executable, os.path.abspath(__file__), "kernel_child",
           "--work", work]
    subprocess.run(cmd, check=True, timeout=LIMIT, cwd=ROOT)
    with open(os.path.join(work, "sequence.json")) as f:
        seq = json.load(f)
    trace = read_trace(work)
    if len(trace) != len(seq["sequence"]):
        raise SystemExit(f"the trace holds {len(trace)} windows-kernel dispatches, the child made {len(seq['sequence'])}")
    lines.append(json.dumps(dict(what="device", library=seq["library"], device=seq["device"], cus=seq["cus"], valu_instructions=VALU_COUNTS)))
    by_label = {}
    for (ms, name), label in zip(trace, seq["sequence"]):
        if label != "untimed":
            want = "sha1_windows_kernel" if label.endswith("sha1_32") else "xxh_windows_kernel"
            assert want in name, (label, name)
            by_label.setdefault(label, []).append(ms)
    for shape in seq["shapes"]:
        rec = dict(what="(a) kernels alone", **shape)
        med = {}
        for label, _, _ in KERNELS:
            ms = by_label[f"{shape['mode']}/{shape['width']}/{label}"]
            assert len(ms) == REPS
            med[label] = float(np.median(ms))
            rec[label + "_kernel_ms"] = [round(x, 4) for x in ms]
            rec[label + "_ns_per_window"] = round(med[label] * 1e6 / shape["windows"], 4)
        for label in ("xxh_32", "xxh_64"):
            rec[label + "_speedup_measured"] = round(med["sha1_32"] / med[label], 2)
            if shape["mode"] == "bytes":  # the counts are those of the byte-shingle instantiations
                rec[label + "_speedup_predicted_from_valu"] = round(VALU_COUNTS["sha1_32"] / VALU_COUNTS[label], 2)
        rec["sha1_32_spread_ms"] = round(max(by_label[f"{shape['mode']}/{shape['width']}/sha1_32"]) - min(by_label[f"{shape['mode']}/{shape['width']}/sha1_32"]), 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)


def main():
    work = os.path.abspath(sys.argv[sys.argv.index("--work") + 1] if "--work" in sys.argv else os.path.join(ROOT, "build", "hashes_bench"))
    os.makedirs(work, exist_ok=True)
    if "kernel_child" in sys.argv:
        return kernel_child(work)
    if "end_to_end_child" in sys.argv:
        return end_to_end_child(work)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "hashes_bench.txt")
    lines = []
    kernels_alone(work, lines)
    subprocess.run([sys.executable, os.path.abspath(__file__), "end_to_end_child", "--work", work], check=True, timeout=LIMIT, cwd=ROOT)
    with open(os.path.join(work, "end_to_end.txt")) as f:
        lines += f.read().splitlines()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
