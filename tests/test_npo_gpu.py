"""No-partitioning hash join (PHT family) on the MI355X: exact match counts and triples.

Expected counts come from the oracle's independent sort-merge counter
(count_join_sort) and from its RHO restatement (rho_join / rho_join_triples): the
cardinality does not depend on the algorithm.  Every comparison is exact."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

DT = np.dtype([("key", "<u4"), ("payload", "<u4")])


def rel(keys):
    keys = np.asarray(keys)
    x = np.empty(len(keys), dtype=DT)
    x["key"] = keys.astype(np.uint64).astype(np.uint32)
    x["payload"] = np.arange(len(keys), dtype=np.uint32)
    return x


def npo(sgx, R, S, **kw):
    return sgx.npo_join(R, len(R), S, len(S), **kw)


def to_dev(x):
    import torch

    return torch.from_numpy(x.view(np.int64)).cuda()


# ------------------------------------------------------------- reference shapes
@pytest.mark.parametrize("n", [1 << 10, 1 << 16, 1 << 20])
def test_reference_pk_fk(sgx, orc, gpu, n):
    R, S = sgx.reference_relations(n, n)
    exp, _ = orc.rho_join(R, S, 4)
    assert exp == n
    res = npo(sgx, R, S)
    assert res.matches == exp
    # a primary-key R of 1..n fills every bucket of next_pow2(n / 2) with exactly two keys,
    # which sit at unrelated positions of the shuffled R: no chain, and a lost slot store
    # (build visibility) is a lost match
    assert res.stats["num_buckets"] == n // 2 and res.stats["overflow_nodes"] == 0
    assert res.stats["ms_total"] > 0


@pytest.mark.parametrize("sel", [50, 10, 1])
def test_fk_sel(sgx, orc, gpu, sel):
    R, S = sgx.reference_relations(1 << 18, 1 << 18, selectivity=sel)
    assert npo(sgx, R, S).matches == orc.rho_join(R, S, 4)[0]


def test_zipf(sgx, orc, gpu):
    n = 1 << 18
    R, S = sgx.reference_relations(n, n, skew=0.75)
    assert npo(sgx, R, S).matches == orc.rho_join(R, S, 4)[0] == n


def test_fk_multiple_copies(sgx, orc, gpu):
    R, S = sgx.reference_relations(1 << 16, 1 << 19)
    assert npo(sgx, R, S).matches == orc.count_join_sort(R, S) == 1 << 19


# ------------------------------------------------------------ tiny and ragged sizes
@pytest.mark.parametrize("nR,nS,kmax", [(3, 5, 2), (1, 1, 0), (2, 1000, 1), (100_003, 77_777, 2**32 - 1),
                                        (5000, 7000, 300)])
def test_tiny_and_ragged(sgx, orc, gpu, nR, nS, kmax):
    rng = np.random.default_rng(nR * 31 + nS)
    R = rel(rng.integers(0, kmax + 1, nR, dtype=np.uint64))
    S = rel(rng.integers(0, kmax + 1, nS, dtype=np.uint64))
    exp = orc.count_join_sort(R, S)
    host = npo(sgx, R, S).matches
    dR, dS = to_dev(R), to_dev(S)
    dev = npo(sgx, dR, dS).matches
    assert host == dev == exp
    if nR > 2:
        # relations that start on an odd tuple (8 but not 16 bytes aligned) and end on one
        assert sgx.npo_join(dR[1:], nR - 1, dS[1:], nS - 1).matches == orc.count_join_sort(R[1:], S[1:])
        assert sgx.npo_join(dR[1:], nR - 2, dS, nS - 1).matches == orc.count_join_sort(R[1:-1], S[:-1])


def test_empty_relations(sgx, gpu):
    R = rel([1, 2, 3])
    assert sgx.npo_join(R, 0, R, 3).matches == 0
    assert sgx.npo_join(R, 3, R, 0).matches == 0
    assert sgx.npo_join(None, 0, None, 0).matches == 0
    assert sgx.last_npo_stats()["matches"] == 0


# ------------------------------------------------------------------ bucket boundary
@pytest.mark.parametrize("b", [4, 10])
@pytest.mark.parametrize("colliding", [2, 3, 4])
def test_bucket_boundary(sgx, orc, gpu, b, colliding):
    """R keys x + i * 2^b share bucket x of a 2^b-bucket table: 2 keys fill it exactly, the
    3rd takes the first overflow node, the 4th the second."""
    x = 5
    rkeys = [x + i * (1 << b) for i in range(colliding)]
    R = rel(rkeys)
    # key i appears i + 1 times in S; same low bits with other high bits match nothing
    skeys = [k for i, k in enumerate(rkeys) for _ in range(i + 1)]
    skeys += [x + i * (1 << b) for i in range(colliding, colliding + 3)] * 2 + [x + (1 << 31), x ^ 1]
    S = rel(np.random.default_rng(b).permutation(np.array(skeys, dtype=np.uint64)))
    exp = sum(range(1, colliding + 1))
    assert orc.count_join_sort(R, S) == exp
    res = npo(sgx, R, S, bucket_bits=b)
    assert res.matches == exp
    assert res.stats["num_buckets"] == 1 << b
    assert res.stats["overflow_nodes"] == max(0, colliding - 2)


@pytest.mark.parametrize("bucket_bits", [0, 1])
def test_one_bucket_holds_everything(sgx, orc, gpu, bucket_bits):
    rng = np.random.default_rng(7)
    rkeys = np.arange(4096, dtype=np.uint64) << 20  # low 20 bits 0: one bucket of 2048 or of 2
    R = rel(rng.permutation(rkeys))
    S = rel(rng.permutation(np.concatenate([rkeys, rkeys[::3], rkeys + 1, rkeys + (1 << 19)])))
    exp = orc.count_join_sort(R, S)
    assert exp == 4096 + len(rkeys[::3])
    res = npo(sgx, R, S, bucket_bits=bucket_bits)
    assert res.matches == exp
    assert res.stats["overflow_nodes"] == 4096 - 2


def test_hot_duplicate(sgx, orc, gpu):
    rng = np.random.default_rng(11)
    hot = 123_456
    R = rel(rng.permutation(np.concatenate([np.full(5000, hot), np.arange(1, 5001) * 7919])))
    sk = rng.integers(0, 40_000, 10_000)
    sk[sk == hot] += 1
    sk[rng.choice(10_000, 7, replace=False)] = hot
    S = rel(sk)
    exp = orc.count_join_sort(R, S)
    assert exp >= 7 * 5000
    assert npo(sgx, R, S).matches == exp


@pytest.mark.parametrize("dup", [1, 3])
def test_keys_zero_and_max(sgx, orc, gpu, dup):
    """0 and 2^32 - 1 are ordinary keys: occupancy comes from the bucket's count."""
    top = 2**32 - 1
    R = rel([0] * dup + [top] * dup + [1, top - 1, 1 << 31])
    S = rel([top, 0, 0, 5, top, top, 1 << 31] * dup)
    exp = orc.count_join_sort(R, S)
    assert exp == dup * dup * 5 + dup
    assert npo(sgx, R, S).matches == exp
    for keys in ([0], [top]):  # alone
        A = rel(keys * dup)
        assert npo(sgx, A, A).matches == dup * dup
        assert npo(sgx, A, rel([k ^ 1 for k in keys])).matches == 0


@pytest.fixture(scope="module")
def dup_relations(orc):
    rng = np.random.default_rng(2)
    big = rel(rng.integers(0, (1 << 12) + 1, 1 << 17))
    small = rel(rng.integers(0, (1 << 12) + 1, 1 << 15))
    return big, small, orc.count_join_sort(big, small)


@pytest.mark.parametrize("bucket_bits", [0, 4, 20])
@pytest.mark.parametrize("r_big", [True, False])
def test_random_with_duplicates(sgx, gpu, dup_relations, r_big, bucket_bits):
    big, small, exp = dup_relations
    R, S = (big, small) if r_big else (small, big)
    assert npo(sgx, R, S, bucket_bits=bucket_bits).matches == exp


# ---------------------------------------------------------------- materialisation
def sorted_triples(t):
    t = np.asarray(t, dtype=np.uint32).reshape(-1, 3)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


@pytest.fixture(scope="module")
def mat_case(orc):
    rng = np.random.default_rng(5)
    n = 1 << 16
    R = rel(rng.integers(0, n // 2, n))
    S = rel(rng.integers(0, n // 2, n))
    exp = sorted_triples(orc.rho_join_triples(R, S, 2))
    assert len(exp) == orc.count_join_sort(R, S) and len(exp) > n
    return R, S, exp


def test_materialize_triples(sgx, gpu, mat_case):
    R, S, exp = mat_case
    m = len(exp)
    out = np.zeros((m, 3), dtype=np.uint32)
    res = npo(sgx, R, S, out=out, out_capacity=m)
    assert res.matches == m
    assert np.array_equal(sorted_triples(out), exp)
    assert res.stats["overflow_nodes"] > 0  # bucket slots and chain nodes both carry payloads


def test_materialize_device_and_host_out_agree(sgx, gpu, mat_case):
    import torch

    R, S, exp = mat_case
    m = len(exp)
    dout = torch.zeros((m, 3), dtype=torch.int32, device="cuda")
    res = sgx.npo_join(to_dev(R), len(R), to_dev(S), len(S), out=dout, out_capacity=m)
    assert res.matches == m
    got = dout.cpu().numpy().view(np.uint32)
    assert np.array_equal(sorted_triples(got), exp)


def test_materialize_tables_dropin(sgx, gpu, mat_case):
    R, S, exp = mat_case
    res = sgx.npo_join_tables(R, len(R), S, len(S), nthreads=2, materialize=True)
    try:
        assert res.totalresults == len(exp) and res.materialized == 1 and res.result_type == 1
        assert res.nthreads == 2 and res.throughput > 0
        assert np.array_equal(sorted_triples(sgx.chunked_table_triples(res)), exp)
    finally:
        sgx.free_result(res)
    cnt = sgx.npo_join_tables(R, len(R), S, len(S))
    assert cnt.totalresults == len(exp) and cnt.materialized == 0 and not cnt.result and cnt.result_type == 0
    js = sgx.rho_stats()
    assert sgx.lib.mi355_last_join_stats(ctypes.byref(js)) == 0
    assert js.matches == len(exp) and js.passes == 0 and js.radix_bits == 0 and js.ms_partition == 0
    assert js.ms_build > 0 and js.ms_probe > 0 and js.ms_total > 0
    assert abs(js.ms_join - js.ms_total) < 1e-9


@pytest.mark.parametrize("device_out", [False, True])
def test_materialize_capacity(sgx, gpu, mat_case, device_out):
    import torch

    R, S, exp = mat_case
    m = len(exp)
    sentinel = 0x5A5A5A5A
    if device_out:
        buf = torch.full((m, 3), sentinel, dtype=torch.int32, device="cuda")
    else:
        buf = np.full((m, 3), sentinel, dtype=np.uint32)
    with pytest.raises(sgx.Mi355Error) as e:
        npo(sgx, R, S, out=buf, out_capacity=m - 1)
    assert e.value.code == sgx.MI355_ERR_CAPACITY and f"{m} triples needed" in str(e.value)
    assert sgx.last_npo_stats()["matches"] == m
    # the element after the m - 1 the buffer was said to hold is untouched
    last = buf[m - 1].cpu().numpy().view(np.uint32) if device_out else buf[m - 1]
    assert (last == sentinel).all()


# ------------------------------------------------------------------------- other
def test_timing_lists_the_launches(sgx, gpu):
    R, S = sgx.reference_relations(1 << 16, 1 << 16)
    res = npo(sgx, R, S, timing=True)
    t = dict(sgx.timings())
    assert {"npo_clear", "npo_build", "npo_probe"} <= set(t)
    assert t["npo_build"] > 0 and t["npo_probe"] > 0
    st = res.stats
    assert st["ms_build"] == t["npo_build"] and st["ms_probe"] == t["npo_probe"] and st["ms_clear"] == t["npo_clear"]
    assert st["ms_total"] > 0 and st["ms_h2d"] > 0
    assert st["table_bytes"] == 16 * st["num_buckets"] and st["max_chain"] == 0


def test_after_release_workspace(sgx, orc, gpu):
    rng = np.random.default_rng(3)
    R = rel(rng.integers(0, 3000, 20_000))
    S = rel(rng.integers(0, 3000, 30_000))
    exp = orc.count_join_sort(R, S)
    assert npo(sgx, R, S).matches == exp  # table and node pool exist
    sgx.release_workspace()
    assert sgx.rho_join(R, len(R), S, len(S)).matches == exp
    assert npo(sgx, R, S).matches == exp


# The rules by which the reference's harness reads a run (SGXv2Scripts/scripts/helpers/
# runner.py:14-55), restated: the second decimal number of the Throughput line, and the
# second-to-last integer (the colour reset ends in 0) of the first phase text in a line.
_PHASE_LINES = [("Total Join Time (cycles)", "total"), ("Partition Overall (cycles)", "partition"),
                ("Build+Join Overall (cycles)", "join_total"), ("Build (cycles)", "build"),
                ("Join (cycles)", "probe")]


def parse_teebench_output(stdout):
    phases, throughput = {}, 0.0
    for line in stdout.splitlines():
        if "Throughput" in line:
            throughput = float(re.findall(r"\d+\.\d+", line)[1])
            continue
        for text, key in _PHASE_LINES:
            if text in line:
                phases[key] = int(re.findall(r"\d+", line)[-2])
                break
    return throughput, phases


NPJ_LINES = ["Total input tuples", "Result tuples", "Total Join Time (cycles)", "Build (cycles)", "Join (cycles)",
             "Cycles-per-tuple", "Total Runtime (us)", "Total RT from TSC (us)", "Throughput (M rec/sec)"]


@pytest.mark.parametrize("alg", ["PHT", "PHT_no", "PHT_un", "PHT_o", "NPO_st", "NPO_no"])
def test_native_driver_binary(gpu, alg):
    exe = os.path.join(PKG, "bin", "native_mi355")
    out = subprocess.run([exe, "-a", alg, "-r", "65536", "-s", "65536"], capture_output=True, text=True, timeout=120,
                         check=True).stdout
    assert "Result tuples : 65536" in out and "Matches = 65536" in out
    pos = [out.index(t) for t in NPJ_LINES]  # the npj print_timing lines, in the reference's order
    assert pos == sorted(pos)
    throughput, phases = parse_teebench_output(out)
    assert throughput > 0
    assert set(phases) == {"total", "build", "probe"}
    assert phases["total"] > 0 and phases["build"] > 0 and phases["probe"] > 0
    assert phases["build"] + phases["probe"] <= phases["total"] + 2


def test_native_driver_unknown_algorithm(gpu):
    exe = os.path.join(PKG, "bin", "native_mi355")
    p = subprocess.run([exe, "-a", "NOPE", "-r", "1024", "-s", "1024"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "Algorithm not found" in p.stdout
