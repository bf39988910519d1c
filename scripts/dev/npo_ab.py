#!/usr/bin/env python3
"""A/Bs of the no-partitioning join's switches, interleaved in one process
(profiles/npo_ab.log): the build's slot/node store form (SGXAMD_NPO_PLAIN) and the
probe's keys in flight (SGXAMD_NPO_KEYS 4 / 8 / 16).  (The log also holds a third A/B,
hipMemsetAsync against a clear kernel; the kernel lost and was removed with its switch.)  Every arm's count is checked; times are the library's event times."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sgxv2-analytical-query-processing-benchmarks_amd", "python"))

import torch  # noqa: E402

import sgxamd  # noqa: E402

ARMS = {
    "store": ("SGXAMD_NPO_PLAIN", {"write_through": "0", "plain": "1"}, "ms_build"),
    "keys": ("SGXAMD_NPO_KEYS", {"4": "4", "8": "8", "16": "16"}, "ms_probe"),
}


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    sgxamd.set_stream(stream)
    for lr, ls, rounds in ((16, 16, 20), (20, 20, 20), (24, 24, 10), (28, 28, 5), (27, 30, 3)):
        nR, nS = 1 << lr, 1 << ls
        R = torch.empty(nR, dtype=torch.int64, device=dev)
        S = torch.empty(nS, dtype=torch.int64, device=dev)
        sgxamd.gen_pk_dev(R, nR, 0, nR, 11111, stream)
        sgxamd.gen_fk_dev(S, nS, 0, nR, 22222, stream)
        torch.cuda.synchronize()
        for what, (env, arms, field) in ARMS.items():
            split = {a: [] for a in arms}
            total = {a: [] for a in arms}
            for rnd in range(rounds + 2):  # two warm-up rounds
                for a, val in arms.items():
                    os.environ[env] = val
                    r = sgxamd.npo_join(R, nR, S, nS, timing=True)
                    assert r.matches == nS, (what, a, r.matches)
                    t = sgxamd.npo_join(R, nR, S, nS)
                    assert t.matches == nS, (what, a, t.matches)
                    if rnd >= 2:
                        split[a].append(r.stat(field))
                        total[a].append(t.stat("ms_total"))
            del os.environ[env]
            for a in arms:
                print(f"2^{lr} x 2^{ls} {what:5s} {a:13s} {field} median {statistics.median(split[a]):.5f} min "
                      f"{min(split[a]):.5f}  | ms_total (one span) median {statistics.median(total[a]):.5f} min "
                      f"{min(total[a]):.5f}  n={rounds}", flush=True)
        del R, S
        sgxamd.release_workspace()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
