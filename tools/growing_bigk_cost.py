#!/usr/bin/env python3
"""growing_bigk_cost.py -- what the growing segment costs a k > 1024 batch on one MI355X, the parent commit's library against this
one in the same call.  C3's corpus (10 M documents, 30 000 terms, generated and indexed on the device as bench.py does) with growing
segments of --sizes (10000,100000) documents of about 60 elements (tests/growing_data.py), the first --queries (64,1024) five-term
queries of its batch, k = 1025, 10000 and 65535.

  python tools/growing_bigk_cost.py profiles/growing_bigk_cost.json --parent <the parent commit's libvbm25.so>

The tool starts two workers, each a process of its own with one of the libraries (VBM25_LIBRARY), and gives them the same commands
in turn: per cell one untimed repetition each, then --reps (5) timed ones alternating parent, new, parent, new ...  A repetition is
the host clock around run + device synchronisation of the batch without a segment (the sealed part) and of the batch with it (the
total); the growing part is the difference.  Medians with min and max, and the CRC of the merged records, which must be equal.  A
gain is stated for a cell only where the margin of the growing part exceeds three times the parent's own max - min spread."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1025, 10000, 65535)


def worker():
    """commands as JSON lines on stdin, one JSON answer a line on stdout"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import vectorchord_bm25_amd as vb
    from bench import WORKLOADS, make_queries
    from growing_data import make_growing

    n_docs, vocab, mean_len, len_mode, zipf_s, _, nterms, _ = WORKLOADS["C3"]
    dseg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
    gix = vb.GpuIndex(dseg)
    all_terms, all_off = make_queries(dseg, vocab, 1024, nterms, seed=3, zipf_s=zipf_s)
    hseg = dseg.download()  # (kept: the arrays are views of it)
    term_key = hseg.arrays()["term_key"]
    st = {}

    def timed(b):
        t0 = time.perf_counter()
        b.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    print(json.dumps({"ready": vb.library_path()}), flush=True)
    for line in sys.stdin:
        c = json.loads(line)
        out = {}
        if c["op"] == "grow":
            st.clear()
            G, _ = make_growing(term_key, c["n"], seed=c["n"], mean_elems=60)
            st["gs"] = vb.GrowingSegment(gix, **G)
        elif c["op"] == "cell":
            for name in ("sealed", "total"):
                st.pop(name, None)
            terms, off = all_terms[:all_off[c["nq"]]], all_off[:c["nq"] + 1]
            for name in ("sealed", "total"):
                b = vb.Batch(gix, c["nq"], len(terms), c["k"])
                if name == "total":
                    b.set_growing(st["gs"])
                b.set_queries(terms, off)
                st[name] = b
        elif c["op"] == "rep":
            out = {"sealed": timed(st["sealed"]), "total": timed(st["total"])}
        elif c["op"] == "records":
            hits, nh = st["total"].fetch()
            n_grow = st["gs"].n_docs
            out = {"records": int(nh.sum()), "records_crc32": zlib.crc32(b"".join(hits[q, :nh[q]].tobytes() for q in range(len(nh)))),
                   "growing_records": int(sum(int((hits[q, :nh[q]]["doc_id"] > 0xFFFFFFFF - n_grow).sum()) for q in range(len(nh))))}
            try:
                out["items_appended_pruned_chunks"] = list(st["total"].debug_bigk_grow())
            except AttributeError:  # (the parent's library has no such route)
                pass
        print(json.dumps(out), flush=True)


def ms(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out", nargs="?")
    p.add_argument("--parent", help="the parent commit's libvbm25.so")
    p.add_argument("--worker", action="store_true")
    p.add_argument("--sizes", default="10000,100000")
    p.add_argument("--queries", default="64,1024")
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    if a.worker:
        return worker()
    if not a.out or not a.parent:
        raise SystemExit("usage: growing_bigk_cost.py OUT.json --parent <the parent commit's libvbm25.so>")
    procs = {}
    for who, lib in (("parent", os.path.abspath(a.parent)), ("new", None)):
        env = dict(os.environ)
        env.pop("VBM25_LIBRARY", None)
        if lib:
            env["VBM25_LIBRARY"] = lib
        procs[who] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=env, stdin=subprocess.PIPE,
                                      stdout=subprocess.PIPE, text=True)

    def ask(who, **cmd):
        if cmd:
            procs[who].stdin.write(json.dumps(cmd) + "\n")
            procs[who].stdin.flush()
        line = procs[who].stdout.readline()
        if not line:
            raise SystemExit(f"the {who} worker ended (exit status {procs[who].wait()})")
        return json.loads(line)

    res = {"unit": "ms", "timed": f"run + device synchronisation, host clock; 1 untimed and {a.reps} timed repetitions, the two libraries alternating",
           "workload": "C3: 10 M documents / 30 000 terms, five-term queries", "libraries": {}}
    try:
        for who in procs:
            with open(ask(who)["ready"], "rb") as f:
                res["libraries"][who] = {"sha256_16": hashlib.sha256(f.read()).hexdigest()[:16]}
        for n in (int(x) for x in a.sizes.split(",")):
            for who in procs:
                ask(who, op="grow", n=n)
            for nq in (int(x) for x in a.queries.split(",")):
                for k in KS:
                    row = {}
                    ts = {who: {"sealed": [], "total": []} for who in procs}
                    for who in procs:
                        ask(who, op="cell", nq=nq, k=k)
                        ask(who, op="rep")  # untimed
                    for _ in range(a.reps):
                        for who in procs:
                            r = ask(who, op="rep")
                            for part in r:
                                ts[who][part].append(r[part])
                    for who in procs:
                        grow = [t - s for t, s in zip(ts[who]["total"], ts[who]["sealed"])]
                        row[who] = dict(sealed=ms(ts[who]["sealed"]), total=ms(ts[who]["total"]), growing=ms(grow), **ask(who, op="records"))
                    pg, ng = row["parent"]["growing"], row["new"]["growing"]
                    row["margin_ms"] = round(pg["median"] - ng["median"], 3)
                    row["parent_spread_ms"] = round(pg["max"] - pg["min"], 3)
                    row["same_records"] = row["parent"]["records_crc32"] == row["new"]["records_crc32"]
                    row["verdict"] = "gain shown" if row["same_records"] and row["margin_ms"] > 3 * row["parent_spread_ms"] else "no gain measured"
                    res.setdefault(f"{n}_growing_documents", {}).setdefault(f"{nq}_queries", {})[str(k)] = row
                    print(f"n_grow={n} nq={nq} k={k}: growing parent {pg} new {ng} -> {row['verdict']}", file=sys.stderr, flush=True)
                    with open(a.out, "w") as f:
                        json.dump(res, f, indent=1)
                        f.write("\n")
    finally:
        for pr in procs.values():
            pr.stdin.close()
        for pr in procs.values():
            pr.wait(timeout=60)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
