#!/usr/bin/env python3
"""sparse_big_cost.py -- what a batch of sparse queries costs at 256 < k <= 1024 on one MI355X: C3's corpus (10 M documents, uniform
vocabulary of 30 000, generated and indexed on the device as bench.py does) and the first --queries (1024) five-term queries of its
batch, at k = 257, 512, 1000 and 1024.  Steps, each a process of its own that adds its part to the JSON file given first:
  --step parent   the yardstick: ANOTHER build of the library -- the parent commit's, given with --library -- on which every query of
                  such a batch takes scan_many_kernel
  --step new      this build with sparse_big=1: the queries through scan_sparse_big_kernel; debug_sparse_big() (items taken, given up
                  for a wide tf, slow-path tiles, cuts) and debug_counts() are recorded beside the times, with the kernel's resources
                  (--resources VGPRS:LDS:SCRATCH, from `make resources`), and the records' CRC must be the parent's
  --step bench    bench.py's results on the paths this change does not touch (C3 at k = 10, C5 at k = 100), several runs a side
Host clock around run + fetch (synchronous), one untimed and --reps (5) timed; median / min / max in ms.  A gain is stated per k only
where the margin exceeds three times the parent route's own max - min spread; anything else is "no gain measured".  Every step under
its own time limit, the second only after the first:

  timeout -k 10 500 python tools/sparse_big_cost.py profiles/sparse_big_cost.json --step parent --library <parent's libvbm25.so> && \\
  timeout -k 10 500 python tools/sparse_big_cost.py profiles/sparse_big_cost.json --step new --resources 115:80648:0"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (257, 512, 1000, 1024)


def ms(ts):
    return {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3)}


def record_bench(a):
    """the paths this change does not touch: bench.py's ms_per_step of several runs a side (the caller alternates them), median / min /
    max, and whether the new median lies inside the parent's min .. max"""
    with open(a.out) as f:
        res = json.load(f)
    runs = {}
    for spec in a.bench:
        name, side, path = spec.split(":", 2)
        line = json.loads(open(path).read().strip().splitlines()[-1])
        runs.setdefault(name, {}).setdefault(side, []).append(line["ms_per_step"] / 1e3)
        runs[name]["workload"] = line["config"]["workload"]
    for name, r in runs.items():
        row = {"workload": r["workload"], "parent": ms(r["parent"]), "new": ms(r["new"]), "runs_a_side": len(r["parent"])}
        row["new_median_inside_parent_spread"] = row["parent"]["min"] <= row["new"]["median"] <= row["parent"]["max"]
        res.setdefault("untouched_paths_bench_py", {})[name] = row
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["untouched_paths_bench_py"]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("--step", choices=("parent", "new", "bench"), required=True)
    p.add_argument("--bench", nargs="*", default=[], metavar="NAME:SIDE:FILE",
                   help="--step bench: output files of bench.py runs (one JSON line each), e.g. C3:parent:c3_p1.json; several a side")
    p.add_argument("--library", help="--step parent: the other build of libvbm25.so")
    p.add_argument("--workload", default="C3")
    p.add_argument("--resources", default="", metavar="VGPRS:LDS:SCRATCH", help="--step new: what the compiler reports for scan_sparse_big_kernel")
    p.add_argument("--queries", type=int, default=1024)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    if a.step == "bench":
        return record_bench(a)
    if (a.step == "parent") != bool(a.library):
        raise SystemExit("--library goes with --step parent, and only with it")
    if a.library:
        os.environ["VBM25_LIBRARY"] = os.path.abspath(a.library)  # (read when the package is imported)
    import vectorchord_bm25_amd as vb
    if a.library:
        assert os.path.samefile(vb.library_path(), a.library)
    from bench import WORKLOADS, make_queries

    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"unit": "ms", "timed": f"run + fetch, host clock, 1 untimed and {a.reps} timed", "workload": a.workload, "queries": a.queries})
    sha = hashlib.sha256(open(vb.library_path(), "rb").read()).hexdigest()[:16]
    if a.step == "new":
        vb.set_tuning("sparse_big", 1)

    n_docs, vocab, mean_len, len_mode, zipf_s, _, nterms, _ = WORKLOADS[a.workload]
    seg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(seg)
    terms, off = make_queries(seg, vocab, 1024, nterms, seed=3, zipf_s=zipf_s)
    terms, off = terms[:off[a.queries]], off[:a.queries + 1]
    part = res.setdefault("by_k", {})
    if a.step == "new" and a.resources:
        vgprs, lds, scratch = (int(x) for x in a.resources.split(":"))
        res["scan_sparse_big_kernel"] = {"vgprs": vgprs, "lds_bytes": lds, "scratch_bytes_per_lane": scratch,
                                         "workgroups_per_cu": min(163840 // lds, 2048 // 512, (512 // ((vgprs + 7) // 8 * 8)) * 4 // 8)}
    for k in KS:
        b = vb.Batch(gix, a.queries, len(terms), k)
        b.set_queries(terms, off)
        ts = []
        for r in range(1 + a.reps):
            t0 = time.perf_counter()
            b.run()
            hits, nh = b.fetch()
            if r:
                ts.append(time.perf_counter() - t0)
        crc = zlib.crc32(b"".join(hits[q, :nh[q]].tobytes() for q in range(a.queries)))
        row = part.setdefault(str(k), {})
        routes, counts = b.debug_routes(), b.debug_counts()
        row[a.step] = dict(ms(ts), library_sha256_16=sha, records=int(nh.sum()), records_crc32=crc, queries_sparse_dense=list(routes[:2]),
                           items_sparse_dense_many=list(routes[3:]), items=counts[0], items_given_up=counts[1])
        if a.step == "new":
            row["new"]["taken_givenup_slowtiles_cuts"] = list(b.debug_sparse_big())
        if "parent" in row and "new" in row:
            spread = row["parent"]["max"] - row["parent"]["min"]
            margin = row["parent"]["median"] - row["new"]["median"]
            row["margin_ms"], row["parent_spread_ms"] = round(margin, 3), round(spread, 3)
            row["same_records"] = row["parent"]["records_crc32"] == row["new"]["records_crc32"]
            row["verdict"] = "gain shown" if margin > 3 * spread else "no gain measured"
        print(f"{a.workload} k={k} {a.step}: {row[a.step]}", file=sys.stderr, flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        del b
    print(json.dumps(res))


if __name__ == "__main__":
    main()
