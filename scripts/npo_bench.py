#!/usr/bin/env python3
"""PHT (no-partitioning join) beside RHO on one MI355X: one process, device-resident
relations, both joins alternating in every round, the library's own event times.

For every size the script reports, over the timed rounds (median and min):
  pht_ms_total   clear + build + probe as one span (timing off: two events per join)
  pht_ms_clear / build / probe   from rounds of their own with per-launch events
                 (an event sits in every gap between two launches, so the spans hold
                 the launches without the gaps: at the small sizes they add up to less
                 than pht_ms_total, which spans the gaps too)
  rho_ms_total   RHO on the same relations (timing off: one span)
and the algorithmic bytes of the PHT kernels with their share of the 8 TB/s
datasheet peak and of the in-tree stream_probe read ceiling measured in this run:
  clear  16 * num_buckets                 (the table, written once)
  build  8 * nR + 8 * nR                  (R read once; per tuple a 4-byte count update and a 4-byte key store)
  probe  8 * nS + 16 * nS                 (S read once; one 16-byte bucket record per S tuple)
These are the bytes the algorithm needs, not the bytes the memory system moves: every
random 4- or 16-byte access costs a whole line beyond the caches.

Prints one JSON line (and writes it to --out).  --store-ab adds the build's
write-through / plain store A/B (SGXAMD_NPO_PLAIN alternating in this process)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgxv2-analytical-query-processing-benchmarks_amd", "python"))

PEAK_GBS = 8000.0  # MI355X datasheet HBM3E bandwidth

CASES = [  # name, log2 |R|, log2 |S|, S generator, timed rounds
    ("2^16", 16, 16, "fk", 30),
    ("2^20 (config 1)", 20, 20, "fk", 30),
    ("2^24", 24, 24, "fk", 15),
    ("2^28 (config 2)", 28, 28, "fk", 7),
    ("2^27 x 2^30 (config 4)", 27, 30, "fk", 5),
    ("2^28 Zipf 0.75", 28, 28, "zipf", 7),
]


def med_min(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-log2", type=int, default=30, help="skip cases with a relation above 2^this")
    ap.add_argument("--store-ab", action="store_true")
    args = ap.parse_args()

    import torch

    import sgxamd

    if not torch.cuda.is_available() or sgxamd.device_count() == 0:
        raise SystemExit("npo_bench needs an MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    sgxamd.set_stream(stream)
    sgxamd.timing_enable(False)

    # read ceiling: the in-tree streaming read kernel over 2 GiB, best of 5 per shape
    nb = 1 << 31
    src = torch.ones(nb // 8, dtype=torch.int64, device=dev)
    dst = torch.zeros(16, dtype=torch.int64, device=dev)
    cur = torch.cuda.Stream()
    cur.wait_stream(torch.cuda.current_stream())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    read_ceiling = 0.0
    for u in (4, 8):
        for grid in (2048, 8192):
            sgxamd.stream_probe("read", src, dst, nb, nt_load=True, loads_in_flight=u, grid=grid, stream=cur.cuda_stream)
            for _ in range(5):
                ev0.record(cur)
                sgxamd.stream_probe("read", src, dst, nb, nt_load=True, loads_in_flight=u, grid=grid,
                                    stream=cur.cuda_stream)
                ev1.record(cur)
                ev1.synchronize()
                read_ceiling = max(read_ceiling, nb / (ev0.elapsed_time(ev1) * 1e-3) / 1e9)
    del src, dst
    torch.cuda.empty_cache()

    def frac(nbytes, ms):
        gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        return {"GB_per_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK_GBS, 4),
                "frac_of_read_ceiling": round(gbs / read_ceiling, 4)}

    sizes = []
    store_ab = []
    for name, lr, ls, gen, rounds in CASES:
        if max(lr, ls) > args.max_log2:
            continue
        nR, nS = 1 << lr, 1 << ls
        R = torch.empty(nR, dtype=torch.int64, device=dev)
        S = torch.empty(nS, dtype=torch.int64, device=dev)
        sgxamd.gen_pk_dev(R, nR, 0, nR, 11111, stream)
        if gen == "zipf":
            sgxamd.gen_zipf_dev(S, nS, 0, nR, 0.75, 22222, stream)
        else:
            sgxamd.gen_fk_dev(S, nS, 0, nR, 22222, stream)
        torch.cuda.synchronize()

        def pht(timing=False):
            r = sgxamd.npo_join(R, nR, S, nS, timing=timing)
            assert r.matches == nS, (name, "PHT", r.matches)
            return r

        def rho():
            r = sgxamd.rho_join(R, nR, S, nS)
            assert r.matches == nS, (name, "RHO", r.matches)
            return r

        for _ in range(args.warmup):
            pht(), rho(), pht(True)
        t = {k: [] for k in ("pht_ms_total", "rho_ms_total", "pht_ms_clear", "pht_ms_build", "pht_ms_probe")}
        for _ in range(rounds):  # PHT and RHO alternate in every round
            p = pht()
            t["pht_ms_total"].append(p.stat("ms_total"))
            t["rho_ms_total"].append(rho().stat("ms_total"))
            p = pht(True)
            for k in ("clear", "build", "probe"):
                t[f"pht_ms_{k}"].append(p.stat(f"ms_{k}"))
        st = p.stats
        row = {"case": name, "nR": nR, "nS": nS, "S": gen, "num_buckets": st["num_buckets"],
               "table_bytes": st["table_bytes"], "overflow_nodes": st["overflow_nodes"]}
        row.update({k: med_min(v) for k, v in t.items()})
        row["rho_over_pht"] = round(row["rho_ms_total"]["median"] / row["pht_ms_total"]["median"], 3)
        row["bytes"] = {"clear": 16 * st["num_buckets"], "build": 16 * nR, "probe": 24 * nS}
        for k in ("clear", "build", "probe"):
            row[f"{k}_rate"] = frac(row["bytes"][k], row[f"pht_ms_{k}"]["median"])
        sizes.append(row)
        print(f"# {name}: PHT {row['pht_ms_total']['median']} ms (clear {row['pht_ms_clear']['median']} build "
              f"{row['pht_ms_build']['median']} probe {row['pht_ms_probe']['median']}), RHO "
              f"{row['rho_ms_total']['median']} ms", file=sys.stderr, flush=True)

        if args.store_ab and lr in (20, 24, 28) and gen == "fk" and lr == ls:
            ab = {"write_through": [], "plain": []}
            for _ in range(rounds):
                for form, env in (("write_through", "0"), ("plain", "1")):
                    os.environ["SGXAMD_NPO_PLAIN"] = env
                    ab[form].append(pht(True).stat("ms_build"))
            os.environ["SGXAMD_NPO_PLAIN"] = "0"
            store_ab.append({"case": name, "build_ms": {k: med_min(v) for k, v in ab.items()},
                             "raw": {k: [round(x, 5) for x in v] for k, v in ab.items()}})
        del R, S
        sgxamd.release_workspace()
        torch.cuda.empty_cache()

    out = {"bench": "npo_bench", "device": torch.cuda.get_device_name(0), "version": sgxamd.version(),
           "how": "one process; device-resident pk R, fk / Zipf S (gen_*_dev, seeds 11111 / 22222); per size "
                  f"{args.warmup} warm-up rounds, then PHT (one span), RHO (one span) and PHT (per-launch events) "
                  "alternating per round; HIP event times of the library; median and min over the rounds",
           "bytes_formula": {"clear": "16 * num_buckets", "build": "8 * nR (R) + 8 * nR (count update + key store)",
                             "probe": "8 * nS (S) + 16 * nS (one bucket record per key)"},
           "peak_GB_per_s": PEAK_GBS, "read_ceiling_GB_per_s": round(read_ceiling, 1),
           "read_ceiling_how": "mi355_stream_probe read, 2 GiB, nt loads, best of 5 over U 4/8 x grid 2048/8192",
           "sizes": sizes}
    if store_ab:
        out["build_store_ab"] = store_ab
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
