#!/usr/bin/env python3
"""The sort-merge join (MWAY / PSM / RSM) beside RHO and PHT on one MI355X: one process,
device-resident relations, the three joins alternating in every round, the library's own
event times.

For every size the script reports, over the timed rounds (median and min):
  smj_ms_total   both sorts + merge as one span (timing off: two events per join; the span
                 holds the host's wait for the digit histograms too)
  smj_ms_sort_r / sort_s / merge and every launch's own time, from rounds with per-launch
                 events (an event sits in every gap, so the spans hold no gaps)
  rho_ms_total / pht_ms_total   RHO and PHT on the same relations (timing off: one span)
the pass counts, and per kernel the algorithmic bytes with their share of the 8 TB/s
datasheet peak and of the in-tree stream_probe copy rate measured in this run
(e = 4 bytes per element for a counting join, n the relation's tuples, P its passes):
  min / digits   8 n each          (the input read; only the key is used)
  tile_hist      P * e n           (first pass: 8 n, the tuples)
  scan           P * 2 * 4 * 256 * tiles
  scatter        P * 2 e n         (first pass: 8 n + e n)
  merge_count    e (nR + nS)       (+ 8 bytes per chunk of splits)
These are the bytes the algorithm needs, not the bytes the memory system moves.

Prints one JSON line (and writes it to --out).  --ab adds the scatter's staged / direct
store A/B (SGXAMD_SMJ_DIRECT alternating in this process)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgxv2-analytical-query-processing-benchmarks_amd", "python"))

PEAK_GBS = 8000.0  # MI355X datasheet HBM3E bandwidth

CASES = [  # name, log2 of the tuples per side, timed rounds
    ("2^16", 16, 30),
    ("2^20", 20, 30),
    ("2^24", 24, 15),
    ("2^28", 28, 7),
]


def med_min(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-log2", type=int, default=28, help="skip cases above 2^this tuples per side")
    ap.add_argument("--ab", action="store_true")
    args = ap.parse_args()

    import torch

    import sgxamd

    if not torch.cuda.is_available() or sgxamd.device_count() == 0:
        raise SystemExit("smj_bench needs an MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    sgxamd.set_stream(stream)
    sgxamd.timing_enable(False)

    # copy rate: the in-tree streaming copy kernel (mi355_stream_probe kind 0), 1 GiB read +
    # 1 GiB written, best of 5 per shape
    nb = 1 << 30
    src = torch.ones(nb // 8, dtype=torch.int64, device=dev)
    dst = torch.zeros(nb // 8, dtype=torch.int64, device=dev)
    cur = torch.cuda.Stream()
    cur.wait_stream(torch.cuda.current_stream())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_rate = 0.0
    for u in (4, 8):
        for grid in (2048, 8192):
            sgxamd.stream_probe("copy", src, dst, nb, loads_in_flight=u, grid=grid, stream=cur.cuda_stream)
            for _ in range(5):
                ev0.record(cur)
                sgxamd.stream_probe("copy", src, dst, nb, loads_in_flight=u, grid=grid, stream=cur.cuda_stream)
                ev1.record(cur)
                ev1.synchronize()
                copy_rate = max(copy_rate, 2 * nb / (ev0.elapsed_time(ev1) * 1e-3) / 1e9)
    del src, dst
    torch.cuda.empty_cache()

    def frac(nbytes, ms):
        gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        return {"bytes": nbytes, "GB_per_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK_GBS, 4),
                "frac_of_copy_rate": round(gbs / copy_rate, 4)}

    sizes, ab_rows = [], []
    for name, lg, rounds in CASES:
        if lg > args.max_log2:
            continue
        n = 1 << lg
        R = torch.empty(n, dtype=torch.int64, device=dev)
        S = torch.empty(n, dtype=torch.int64, device=dev)
        sgxamd.gen_pk_dev(R, n, 0, n, 11111, stream)
        sgxamd.gen_fk_dev(S, n, 0, n, 22222, stream)
        torch.cuda.synchronize()

        def smj(timing=False):
            r = sgxamd.smj_join(R, n, S, n, timing=timing)
            assert r.matches == n, (name, "SMJ", r.matches)
            return r

        def rho():
            r = sgxamd.rho_join(R, n, S, n)
            assert r.matches == n, (name, "RHO", r.matches)
            return r

        def pht():
            r = sgxamd.npo_join(R, n, S, n)
            assert r.matches == n, (name, "PHT", r.matches)
            return r

        for _ in range(args.warmup):
            smj(), rho(), pht(), smj(True)
        t = {k: [] for k in ("smj_ms_total", "rho_ms_total", "pht_ms_total", "smj_ms_sort_r", "smj_ms_sort_s",
                             "smj_ms_merge")}
        launches = {}
        for _ in range(rounds):  # SMJ, RHO and PHT alternate in every round
            t["smj_ms_total"].append(smj().stat("ms_total"))
            t["rho_ms_total"].append(rho().stat("ms_total"))
            t["pht_ms_total"].append(pht().stat("ms_total"))
            p = smj(True)
            for k in ("sort_r", "sort_s", "merge"):
                t[f"smj_ms_{k}"].append(p.stat(f"ms_{k}"))
            per = {}
            for nm, ms in sgxamd.timings():  # the passes of one kernel and relation, summed
                per[nm] = per.get(nm, 0.0) + ms
            for nm, ms in per.items():
                launches.setdefault(nm, []).append(ms)
        st = p.stats
        e, tile = st["elem_bytes"], st["sort_tile"]
        row = {"case": name, "nR": n, "nS": n, "sort_passes_r": st["sort_passes_r"],
               "sort_passes_s": st["sort_passes_s"], "elem_bytes": e, "sort_tile": tile,
               "merge_tile": st["merge_tile"]}
        row.update({k: med_min(v) for k, v in t.items()})
        row["smj_over_rho"] = round(row["smj_ms_total"]["median"] / row["rho_ms_total"]["median"], 3)
        row["smj_over_pht"] = round(row["smj_ms_total"]["median"] / row["pht_ms_total"]["median"], 3)
        tiles = (n + tile - 1) // tile
        kern = {}
        for side in ("r", "s"):
            P = st[f"sort_passes_{side}"]
            b = {"min": 8 * n, "digits": 8 * n, "hist": 8 * n + (P - 1) * e * n if P else 0,
                 "scan": P * 2 * 4 * 256 * tiles, "scatter": (8 + e) * n + (P - 1) * 2 * e * n if P else 0}
            for k, nbytes in b.items():
                nm = f"smj_sort_{side}_{k}"
                if nm in launches:
                    kern[nm] = {"ms": med_min(launches[nm]), **frac(nbytes, statistics.median(launches[nm]))}
        for nm, nbytes in (("smj_merge_partition", 8 * ((2 * n + st["merge_tile"] - 1) // st["merge_tile"] + 1)),
                           ("smj_merge_count", e * 2 * n)):
            kern[nm] = {"ms": med_min(launches[nm]), **frac(nbytes, statistics.median(launches[nm]))}
        row["kernels"] = kern
        sizes.append(row)
        print(f"# {name}: SMJ {row['smj_ms_total']['median']} ms (sort R {row['smj_ms_sort_r']['median']} sort S "
              f"{row['smj_ms_sort_s']['median']} merge {row['smj_ms_merge']['median']}; passes {st['sort_passes_r']}"
              f"+{st['sort_passes_s']}), RHO {row['rho_ms_total']['median']} ms, PHT "
              f"{row['pht_ms_total']['median']} ms", file=sys.stderr, flush=True)

        if args.ab and lg >= 20:
            ab = {"staged": [], "direct": []}
            for _ in range(rounds):
                for form, env in (("staged", "0"), ("direct", "1")):
                    os.environ["SGXAMD_SMJ_DIRECT"] = env
                    smj(True)
                    ab[form].append(sum(ms for nm, ms in sgxamd.timings() if nm.endswith("_scatter")))
            os.environ["SGXAMD_SMJ_DIRECT"] = "0"
            ab_rows.append({"case": name, "scatter_ms": {k: med_min(v) for k, v in ab.items()},
                            "raw": {k: [round(x, 5) for x in v] for k, v in ab.items()}})
            print(f"# {name}: scatter staged {ab_rows[-1]['scatter_ms']['staged']['median']} ms, direct "
                  f"{ab_rows[-1]['scatter_ms']['direct']['median']} ms", file=sys.stderr, flush=True)
        del R, S
        sgxamd.release_workspace()
        torch.cuda.empty_cache()

    out = {"bench": "smj_bench", "device": torch.cuda.get_device_name(0), "version": sgxamd.version(),
           "how": "one process; device-resident pk R, fk S (gen_*_dev, seeds 11111 / 22222); per size "
                  f"{args.warmup} warm-up rounds, then SMJ (one span), RHO (one span), PHT (one span) and SMJ "
                  "(per-launch events) alternating per round; HIP event times of the library; median and min over "
                  "the rounds; a kernel's ms is the sum over the relation's passes",
           "peak_GB_per_s": PEAK_GBS, "copy_rate_GB_per_s": round(copy_rate, 1),
           "copy_rate_how": "mi355_stream_probe copy (kind 0), 1 GiB read + 1 GiB written, nt accesses, best of 5 "
                            "over U 4/8 x grid 2048/8192",
           "sizes": sizes}
    if ab_rows:
        out["scatter_ab"] = ab_rows
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
