#!/usr/bin/env python3
"""bigk_cost.py -- what a k > 1024 batch costs on one MI355X: C3's corpus (10 M documents, 30 000 terms, generated and indexed on the
device as bench.py does) and the first --queries (64,1024: one section of the file each) five-term queries of its batch, at k = 1025,
2000, 10000 and 65535.  Steps, each a process of its own that adds its part to the JSON file given first:
  --step parent   the yardstick: ANOTHER build of the library -- the parent commit's, given with --library
  --step new      this build; Batch.bigk_queries() and Batch.debug_bigk_win() (items of the window scan, items of the block scan,
                  slow-path tiles, wide postings decoded) are recorded beside the times, and the records' CRC must be the parent's.
                  --dense on both steps: C5's shape (50 M documents, Zipf(1) vocabulary of 100 000, the first 8 and the first 64
                  ten-term queries) at the same four k -- the dense queries of bigk_dense.h against the per-query path they had;
                  Batch.debug_bigk_dense() (dense queries batched, levels, clip-bin boundaries, candidates listed) is recorded.
                  --skip-c3: only that part.
  --step tile     a build with another compile-time tile span of bigk_scan_win_kernel (make variant UNIT=bigk.hip
                  EXTRA=-DVBM25_BIGK_WIN_G=n, given with --library; without: this build), recorded under --label
Host clock around run + fetch (synchronous), one untimed and --reps (5) timed; median / min / max in ms.  A gain is stated per k only
where the margin exceeds three times the parent route's own max - min spread; anything else is "no gain measured".  Every step under
its own time limit, each only after the one before:

  timeout -k 10 500 python tools/bigk_cost.py profiles/bigk_win_cost.json --step parent --library <parent's libvbm25.so> && \\
  timeout -k 10 500 python tools/bigk_cost.py profiles/bigk_win_cost.json --step new"""
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

KS = (1025, 2000, 10000, 65535)


def ms(ts):
    return {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("--step", choices=("parent", "new", "tile"), required=True)
    p.add_argument("--library", help="--step parent / tile: the other build of libvbm25.so")
    p.add_argument("--label", help="--step tile: the name of the build in the file, e.g. g4")
    p.add_argument("--queries", default="64,1024")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--dense", action="store_true", help="also C5's shape, 8 and 64 queries (a minute of generation)")
    p.add_argument("--skip-c3", action="store_true", help="with --dense: C5's shape only")
    a = p.parse_args()
    if (a.step == "parent" and not a.library) or (a.step == "new" and a.library) or (a.step == "tile") != bool(a.label):
        raise SystemExit("--library goes with --step parent (and may with tile), --label with --step tile")
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
    res.update({"unit": "ms", "timed": f"run + fetch, host clock, 1 untimed and {a.reps} timed"})
    sha = hashlib.sha256(open(vb.library_path(), "rb").read()).hexdigest()[:16]
    who = a.label or a.step

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def measure(name, nqs, ks, section):
        n_docs, vocab, mean_len, len_mode, zipf_s, _, nterms, _ = WORKLOADS[name]
        seg = vb.DeviceSegment.synth(n_docs, vocab, mean_len=mean_len, len_mode=len_mode, zipf_s=zipf_s, seed=20260925, device=0)
        gix = vb.GpuIndex(seg)
        all_terms, all_off = make_queries(seg, vocab, 1024, nterms, seed=3, zipf_s=zipf_s)
        for nq in nqs:
            part = res.setdefault(section.format(nq), {})
            terms, off = all_terms[:all_off[nq]], all_off[:nq + 1]
            for k in ks:
                b = vb.Batch(gix, nq, len(terms), k)
                b.set_queries(terms, off)
                ts = []
                for r in range(1 + a.reps):
                    t0 = time.perf_counter()
                    b.run()
                    hits, nh = b.fetch()
                    if r:
                        ts.append(time.perf_counter() - t0)
                crc = zlib.crc32(b"".join(hits[q, :nh[q]].tobytes() for q in range(nq)))
                row = part.setdefault(str(k), {})
                row[who] = dict(ms(ts), library_sha256_16=sha, records=int(nh.sum()), records_crc32=crc,
                                queries_sparse_fallback=list(b.bigk_queries()))
                if a.step != "parent":
                    row[who]["items_win_blk_slowtiles_wide"] = list(b.debug_bigk_win())
                    row[who]["dense_queries_levels_clips_candidates"] = list(b.debug_bigk_dense())
                if "parent" in row and "new" in row:
                    spread = row["parent"]["max"] - row["parent"]["min"]
                    margin = row["parent"]["median"] - row["new"]["median"]
                    row["margin_ms"], row["parent_spread_ms"] = round(margin, 3), round(spread, 3)
                    row["same_records"] = all(v["records_crc32"] == row["parent"]["records_crc32"] for v in row.values() if isinstance(v, dict))
                    row["verdict"] = "gain shown" if margin > 3 * spread else "no gain measured"
                print(f"{name} {nq} queries k={k} {who}: {row[who]}", file=sys.stderr, flush=True)
                save()
                del b

    if not (a.dense and a.skip_c3):
        measure("C3", [int(x) for x in a.queries.split(",")], KS, "c3_{}_queries")
    if a.dense:
        measure("C5", [8, 64], KS, "c5_dense_{}_queries")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
