"""Sort-merge join (MWAY / PSM / RSM) and the device-wide radix sort on the MI355X.

Every comparison is exact.  Expected counts come from the oracle's sort-merge counter
(count_join_sort) and its RHO restatement (rho_join), expected triples from
rho_join_triples (as multisets), the expected sort order from numpy's stable argsort.
Shapes are built from the tile sizes the library reports (sort_tile, merge_tile), so they
sit on the kernels' real boundaries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

DT = np.dtype([("key", "<u4"), ("payload", "<u4")])
TOP = 2**32 - 1


def rel(keys):
    keys = np.asarray(keys)
    x = np.empty(len(keys), dtype=DT)
    x["key"] = keys.astype(np.uint64).astype(np.uint32)
    x["payload"] = np.arange(len(keys), dtype=np.uint32)
    return x


def smj(sgx, R, S, **kw):
    return sgx.smj_join(R, len(R), S, len(S), **kw)


def to_dev(x):
    import torch

    return torch.from_numpy(x.view(np.int64)).cuda()


def shuffled(rng, keys):
    return rel(rng.permutation(np.asarray(keys, dtype=np.uint64)))


@pytest.fixture(scope="module")
def tiles(sgx, gpu):
    """(sort_tile, merge_tile): the geometry the library reports."""
    st = smj(sgx, rel([1, 2]), rel([2, 3])).stats
    assert st["sort_tile"] >= 64 and st["merge_tile"] >= 64
    return st["sort_tile"], st["merge_tile"]


# ------------------------------------------------------------------------ sort alone
def varying_digits(keys):
    """Radix passes a sort of `keys` needs: the bytes of key - min(key) that differ between
    keys.  With key 0 present these are the non-constant bytes of the keys themselves."""
    if len(keys) == 0:
        return 0
    k = keys.astype(np.uint64) - np.uint64(keys.min())
    return sum(len(np.unique((k >> np.uint64(8 * p)) & np.uint64(255))) > 1 for p in range(4))


def raw_varying_digits(keys):
    k = keys.astype(np.uint64)
    return sum(len(np.unique((k >> np.uint64(8 * p)) & np.uint64(255))) > 1 for p in range(4))


def pattern_keys(pattern, n, rng):
    """Keys of one pattern and, for n >= 2, the passes the issue names for it."""
    if pattern == "full32":
        k = rng.integers(0, 2**32, n, dtype=np.uint64)
        if n >= 2:
            k[rng.integers(0, n // 2)] = 0
            k[n // 2 + rng.integers(0, n - n // 2)] = TOP
        return k, 4
    if pattern in ("lt8", "lt16", "shl24"):
        k = rng.integers(0, 1 << (16 if pattern == "lt16" else 8), n, dtype=np.uint64)
        if n >= 2:
            k[n // 2] = 0
            k[n // 2 - 1] = 0xFFFF if pattern == "lt16" else 0xFF
        return (k << np.uint64(24), 1) if pattern == "shl24" else (k, 2 if pattern == "lt16" else 1)
    if pattern == "equal":
        return np.full(n, 0xDEADBEEF, dtype=np.uint64), 0
    k = (np.arange(n, dtype=np.uint64) // 2) * 5  # duplicates: stability shows in the payloads
    return (k if pattern == "ascending" else k[::-1].copy()), None


@pytest.mark.parametrize("pattern", ["full32", "lt8", "lt16", "shl24", "equal", "ascending", "descending"])
def test_sort_rows(sgx, gpu, tiles, pattern):
    import torch

    T = tiles[0]
    rng = np.random.default_rng(len(pattern))
    for n in [1, 2, 255, T - 1, T, T + 1, 3 * T + 17, 1 << 20]:
        keys, named = pattern_keys(pattern, n, rng)
        x = rel(keys)
        exp = x[np.argsort(x["key"], kind="stable")]
        want = varying_digits(x["key"])
        if pattern not in ("ascending", "descending"):
            assert want == raw_varying_digits(x["key"])  # key 0 is present: the keys' own digits
        if named is not None and n >= 255:
            assert want == named, (pattern, n)
        # host in, host out
        out = np.zeros(n, dtype=DT)
        assert sgx.sort_rows(x, n, out) == want, (pattern, n)
        assert np.array_equal(out.view(np.uint64), exp.view(np.uint64)), (pattern, n)
        # device in, device out; the input is bit-identical afterwards
        dx = to_dev(x)
        dout = torch.zeros(n, dtype=torch.int64, device="cuda")
        assert sgx.sort_rows(dx, n, dout) == want
        assert np.array_equal(dout.cpu().numpy().view(np.uint64), exp.view(np.uint64)), (pattern, n)
        assert np.array_equal(dx.cpu().numpy().view(np.uint64), x.view(np.uint64))
        # an odd start (8 but not 16 bytes aligned) on both sides, device in and host out
        if n >= 3:
            y = x[1:]
            expy = y[np.argsort(y["key"], kind="stable")]
            dout.zero_()
            assert sgx.sort_rows(dx[1:], n - 1, dout[1:]) == varying_digits(y["key"])
            got = dout.cpu().numpy().view(np.uint64)
            assert got[0] == 0 and np.array_equal(got[1:], expy.view(np.uint64)), (pattern, n)
            hout = np.zeros(n - 1, dtype=DT)
            sgx.sort_rows(dx[1:], n - 1, hout)
            assert np.array_equal(hout.view(np.uint64), expy.view(np.uint64))


# ------------------------------------------------------------------ reference shapes
@pytest.mark.parametrize("n,passes_r", [(1 << 10, 2), (1 << 16, 2), (1 << 20, 3)])
def test_reference_pk_fk(sgx, orc, gpu, n, passes_r):
    R, S = sgx.reference_relations(n, n)
    exp, _ = orc.rho_join(R, S, 4)
    assert exp == n
    res = smj(sgx, R, S)
    assert res.matches == exp == len(S)
    st = res.stats
    assert st["sort_passes_r"] == passes_r and st["sort_passes_s"] == varying_digits(S["key"])
    assert st["elem_bytes"] == 4 and st["ms_total"] > 0


@pytest.mark.parametrize("sel", [50, 10, 1])
def test_fk_sel(sgx, orc, gpu, sel):
    R, S = sgx.reference_relations(1 << 18, 1 << 18, selectivity=sel)
    assert smj(sgx, R, S).matches == orc.rho_join(R, S, 4)[0]


def test_zipf(sgx, orc, gpu):
    n = 1 << 18
    R, S = sgx.reference_relations(n, n, skew=0.75)
    assert smj(sgx, R, S).matches == orc.rho_join(R, S, 4)[0] == n


def test_fk_multiple_copies(sgx, orc, gpu):
    R, S = sgx.reference_relations(1 << 16, 1 << 19)
    assert smj(sgx, R, S).matches == orc.count_join_sort(R, S) == 1 << 19


# ------------------------------------------------------------ tiny and ragged sizes
@pytest.mark.parametrize("nR,nS,kmax", [(3, 5, 2), (1, 1, 0), (2, 1000, 1), (100_003, 77_777, 2**32 - 1),
                                        (5000, 7000, 300)])
def test_tiny_and_ragged(sgx, orc, gpu, nR, nS, kmax):
    rng = np.random.default_rng(nR * 31 + nS)
    R = rel(rng.integers(0, kmax + 1, nR, dtype=np.uint64))
    S = rel(rng.integers(0, kmax + 1, nS, dtype=np.uint64))
    exp = orc.count_join_sort(R, S)
    host = smj(sgx, R, S).matches
    dR, dS = to_dev(R), to_dev(S)
    dev = smj(sgx, dR, dS).matches
    assert host == dev == exp
    assert np.array_equal(dR.cpu().numpy().view(np.uint64), R.view(np.uint64))  # inputs are never modified
    assert np.array_equal(dS.cpu().numpy().view(np.uint64), S.view(np.uint64))
    if nR > 2:
        # relations that start on an odd tuple (8 but not 16 bytes aligned) and end on one
        assert sgx.smj_join(dR[1:], nR - 1, dS[1:], nS - 1).matches == orc.count_join_sort(R[1:], S[1:])
        assert sgx.smj_join(dR[1:], nR - 2, dS, nS - 1).matches == orc.count_join_sort(R[1:-1], S[:-1])


def test_empty_relations(sgx, gpu):
    R = rel([1, 2, 3])
    assert sgx.smj_join(R, 0, R, 3).matches == 0
    assert sgx.smj_join(R, 3, R, 0).matches == 0
    assert sgx.smj_join(None, 0, None, 0).matches == 0
    assert sgx.last_smj_stats()["matches"] == 0


# --------------------------------------------------------------------- run boundaries
def tile_sizes(tiles):
    return sorted(set(tiles))


@pytest.mark.parametrize("hot", ["middle", "smallest", "largest"])
@pytest.mark.parametrize("run_in", ["S", "R"])
def test_long_run_against_one_copy(sgx, orc, gpu, tiles, hot, run_in):
    """One relation holds a key 3T + 5 times, the other once among T other keys: the run
    crosses sort tiles and merge chunks and is counted once."""
    for T in tile_sizes(tiles):
        rng = np.random.default_rng(T)
        h = {"middle": 1 << 20, "smallest": 0, "largest": TOP}[hot]
        others = (np.arange(1, T + 1, dtype=np.uint64) * 977) + (0 if hot != "middle" else 0)
        others = others[others != h]
        single = shuffled(rng, np.concatenate([[h], others]))
        run = shuffled(rng, np.concatenate([np.full(3 * T + 5, h, dtype=np.uint64), others[::7], others[::5] + 1]))
        R, S = (single, run) if run_in == "S" else (run, single)
        exp = orc.count_join_sort(R, S)
        assert exp == 3 * T + 5 + len(others[::7]) + int(np.isin(others[::5] + 1, others).sum())
        assert smj(sgx, R, S).matches == exp, (T, hot, run_in)


@pytest.mark.parametrize("first_of_run", ["R", "S"])
def test_run_starts_on_last_element_of_a_chunk(sgx, orc, gpu, tiles, first_of_run):
    """In the merged sequence (R before S on equal keys) the element T - 1, the last of
    chunk 0, is the first element of key h's R run, or of its S run."""
    for T in tile_sizes(tiles):
        rng = np.random.default_rng(T + 1)
        h = 10 * T
        small = T - 1 if first_of_run == "R" else T - 6  # R keys below h: then 5 copies of h
        R = shuffled(rng, np.concatenate([np.arange(1, small + 1), np.full(5, h)]))
        S = shuffled(rng, np.concatenate([np.full(7, h), [h + 1, h + 2]]))
        assert orc.count_join_sort(R, S) == 35
        assert smj(sgx, R, S).matches == 35, (T, first_of_run)
        assert smj(sgx, S, R).matches == 35


def test_count_beyond_32_bits(sgx, gpu):
    """2^16 copies of one key on each side: exactly 2^32 matches, from run lengths."""
    k = 0x12345678
    A = rel(np.full(1 << 16, k, dtype=np.uint64))
    res = smj(sgx, A, A)
    assert res.matches == 1 << 32
    assert res.stats["sort_passes_r"] == 0 and res.stats["sort_passes_s"] == 0
    # the same run beside other keys: the sorts run, the count stays
    rng = np.random.default_rng(9)
    B = shuffled(rng, np.concatenate([np.full(1 << 16, k, dtype=np.uint64), np.arange(100, 1100)]))
    C = shuffled(rng, np.concatenate([np.full(1 << 16, k, dtype=np.uint64), np.arange(600, 1600)]))
    assert smj(sgx, B, C).matches == (1 << 32) + 500


def test_one_s_tile_spans_all_of_r(sgx, orc, gpu, tiles):
    """S holds only keys 0 and 2^32 - 1, one tile of them; R is 2^18 distinct keys that
    include both: every chunk of R lies between the two S runs."""
    T = max(tiles)
    rng = np.random.default_rng(4)
    rk = np.unique(np.concatenate([rng.integers(1, TOP, (1 << 18) - 2, dtype=np.uint64), [0, TOP]]))
    R = shuffled(rng, rk)
    S = shuffled(rng, np.concatenate([np.zeros(T // 2, dtype=np.uint64), np.full(T - T // 2, TOP, dtype=np.uint64)]))
    assert orc.count_join_sort(R, S) == T
    assert smj(sgx, R, S).matches == T
    assert smj(sgx, S, R).matches == T


# ---------------------------------------------------------------- materialisation
def sorted_triples(t):
    t = np.asarray(t, dtype=np.uint32).reshape(-1, 3)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


@pytest.fixture(scope="module")
def mat_case(orc):
    rng = np.random.default_rng(5)
    R = rel(rng.integers(0, 301, 5000))
    S = rel(rng.integers(0, 301, 7000))
    exp = sorted_triples(orc.rho_join_triples(R, S, 2))
    assert len(exp) == orc.count_join_sort(R, S) and len(exp) > 7000
    return R, S, exp


def test_materialize_triples(sgx, gpu, mat_case):
    R, S, exp = mat_case
    m = len(exp)
    out = np.zeros((m, 3), dtype=np.uint32)
    res = smj(sgx, R, S, out=out, out_capacity=m)
    assert res.matches == m and res.stats["elem_bytes"] == 8
    assert np.array_equal(sorted_triples(out), exp)


def test_materialize_pk_fk(sgx, orc, gpu):
    n = 1 << 16
    R, S = sgx.reference_relations(n, n)
    exp = sorted_triples(orc.rho_join_triples(R, S, 2))
    assert len(exp) == n
    out = np.zeros((n, 3), dtype=np.uint32)
    assert smj(sgx, R, S, out=out, out_capacity=n).matches == n
    assert np.array_equal(sorted_triples(out), exp)


def test_materialize_device_and_host_out_agree(sgx, gpu, mat_case):
    import torch

    R, S, exp = mat_case
    m = len(exp)
    dout = torch.zeros((m, 3), dtype=torch.int32, device="cuda")
    res = sgx.smj_join(to_dev(R), len(R), to_dev(S), len(S), out=dout, out_capacity=m)
    assert res.matches == m
    got = dout.cpu().numpy().view(np.uint32)
    assert np.array_equal(sorted_triples(got), exp)


def test_materialize_tables_dropin(sgx, gpu, mat_case):
    R, S, exp = mat_case
    res = sgx.smj_join_tables(R, len(R), S, len(S), nthreads=2, materialize=True)
    try:
        assert res.totalresults == len(exp) and res.materialized == 1 and res.result_type == 1
        assert res.nthreads == 2 and res.throughput > 0
        assert np.array_equal(sorted_triples(sgx.chunked_table_triples(res)), exp)
    finally:
        sgx.free_result(res)
    cnt = sgx.smj_join_tables(R, len(R), S, len(S))
    assert cnt.totalresults == len(exp) and cnt.materialized == 0 and not cnt.result and cnt.result_type == 0
    js = sgx.rho_stats()
    assert sgx.lib.mi355_last_join_stats(ctypes.byref(js)) == 0
    sm = sgx.last_smj_stats()
    assert js.matches == len(exp) and js.passes == 0 and js.radix_bits == 0 and js.ms_build == 0
    assert js.ms_partition == sm["ms_sort_r"] + sm["ms_sort_s"] > 0 and js.ms_join == sm["ms_merge"] > 0
    assert js.ms_total == sm["ms_total"] > 0


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
        smj(sgx, R, S, out=buf, out_capacity=m - 1)
    assert e.value.code == sgx.MI355_ERR_CAPACITY and f"{m} triples needed" in str(e.value)
    assert sgx.last_smj_stats()["matches"] == m
    # nothing was written
    whole = buf.cpu().numpy().view(np.uint32) if device_out else buf
    assert (whole == sentinel).all()


# ------------------------------------------------------------------- sorted flags
@pytest.mark.parametrize("side", ["R", "S", "both"])
def test_sorted_flags(sgx, orc, gpu, side):
    rng = np.random.default_rng(12)
    R = rel(rng.integers(0, 1 << 20, 50_000))
    S = rel(rng.integers(0, 1 << 20, 70_001))
    exp = orc.count_join_sort(R, S)
    plain = smj(sgx, R, S, timing=True)
    launches = len(sgx.timings())
    assert plain.matches == exp and plain.stats["sort_passes_r"] == 3 and plain.stats["sort_passes_s"] == 3
    rs, ss = side in ("R", "both"), side in ("S", "both")
    Rs = R[np.argsort(R["key"], kind="stable")] if rs else R
    Ss = S[np.argsort(S["key"], kind="stable")] if ss else S
    for dev in (False, True):
        a, b = (to_dev(Rs), to_dev(Ss)) if dev else (Rs, Ss)
        res = sgx.smj_join(a, len(R), b, len(S), r_sorted=rs, s_sorted=ss, timing=True)
        assert res.matches == exp
        assert res.stats["sort_passes_r"] == (0 if rs else 3) and res.stats["sort_passes_s"] == (0 if ss else 3)
        assert len(sgx.timings()) < launches
    out = np.zeros((exp, 3), dtype=np.uint32)
    assert sgx.smj_join(Rs, len(R), Ss, len(S), r_sorted=rs, s_sorted=ss, out=out, out_capacity=exp).matches == exp
    assert np.array_equal(sorted_triples(out), sorted_triples(orc.rho_join_triples(R, S, 2)))
    t = sgx.smj_join_tables(Rs, len(R), Ss, len(S), r_sorted=rs, s_sorted=ss)
    assert t.totalresults == exp
    assert sgx.last_smj_stats()["sort_passes_r"] == (0 if rs else 3)


def test_timing_lists_the_launches(sgx, gpu):
    R, S = sgx.reference_relations(1 << 16, 1 << 16)
    res = smj(sgx, R, S, timing=True)
    names = [n for n, _ in sgx.timings()]
    st = res.stats
    for side, p in (("r", st["sort_passes_r"]), ("s", st["sort_passes_s"])):
        for k in ("hist", "scan", "scatter"):
            assert names.count(f"smj_sort_{side}_{k}") == p
        assert names.count(f"smj_sort_{side}_digits") == 1
    assert names.count("smj_merge_partition") == 1 and names.count("smj_merge_count") == 1
    assert st["ms_sort_r"] > 0 and st["ms_sort_s"] > 0 and st["ms_merge"] > 0 and st["ms_h2d"] > 0
    assert abs(st["ms_total"] - (st["ms_sort_r"] + st["ms_sort_s"] + st["ms_merge"])) < 1e-9


# ------------------------------------------------------------------------ drop-ins
RUN_JOIN = "_Z8run_joinP8result_tPK7table_tS3_PKcPK12joinconfig_t"


@pytest.mark.parametrize("alg", ["MWAY", "PSM", "RSM"])
def test_run_join_by_name(sgx, orc, gpu, alg):
    rng = np.random.default_rng(21)
    R = rel(rng.integers(0, 5000, 20_000))
    S = rel(rng.integers(0, 5000, 30_000))
    fn = getattr(sgx.lib, RUN_JOIN)
    fn.restype = None
    fn.argtypes = [ctypes.POINTER(sgx.result_t), ctypes.POINTER(sgx.table_t), ctypes.POINTER(sgx.table_t),
                   ctypes.c_char_p, ctypes.POINTER(sgx.joinconfig_t)]
    tR, tS = sgx.table_t(sgx.ptr(R), len(R), 0, 0), sgx.table_t(sgx.ptr(S), len(S), 0, 0)
    cfg = sgx.joinconfig_t()
    cfg.NTHREADS = 3
    res = sgx.result_t()
    fn(ctypes.byref(res), ctypes.byref(tR), ctypes.byref(tS), alg.encode(), ctypes.byref(cfg))
    assert res.totalresults == orc.count_join_sort(R, S) and res.nthreads == 3 and res.materialized == 0


# The rules by which the reference's harness reads a run (SGXv2Scripts/scripts/helpers/
# runner.py:14-55), restated: the second decimal number of the Throughput line, and the
# second-to-last integer (the colour reset ends in 0) of the first phase text in a line.
_PHASE_LINES = [("Total Join Time (cycles)", "total"), ("Partition Overall (cycles)", "partition"),
                ("Partition Pass One (cycles)", "partition_1"), ("Partition One Hist (cycles)", "partition_r"),
                ("Partition One Copy (cycles)", "partition_s"), ("Partition Pass Two (cycles)", "partition_2"),
                ("Partition Two Hist (cycles)", "partition_2_h"), ("Partition Two Copy (cycles)", "partition_2_c"),
                ("Build+Join Overall (cycles)", "join_total"), ("Build (cycles)", "build"),
                ("Join (cycles)", "probe")]


def parse_teebench_output(stdout):
    import re

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


PSM_LINES = ["Total input tuples", "Result tuples", "Total Join Time (cycles)", "Partition Overall (cycles)",
             "Build+Join Overall (cycles)", "Cycles-per-tuple  ", "Cycles-per-tuple-partition",
             "Cycles-per-tuple-join", "Total Runtime (us)", "Total RT from TSC (us)", "Throughput (M rec/sec)"]
RADIX_LINES = ["Total input tuples", "Result tuples", "Total Join Time (cycles)", "Partition Overall (cycles)",
               "Partition Pass One (cycles)", "Partition Pass Two (cycles)", "Build+Join Overall (cycles)",
               "Build (cycles)", "Join (cycles)", "Cycles-per-tuple  ", "Cycles-per-tuple-partition ",
               "Cycles-per-tuple-partitioning_pass_1_timer", "Cycles-per-tuple-partitioning_pass_2_timer",
               "Cycles-per-tuple-join", "Pure Join Runtime (us)", "Throughput (M rec/sec)", "Total Runtime (us)"]


@pytest.mark.parametrize("alg,extra", [("MWAY", []), ("PSM", []), ("RSM", []), ("MWAY", ["-m"]),
                                       ("PSM", ["--sort-r"]), ("RSM", ["-m", "--sort-r", "--sort-s"])])
def test_native_driver_binary(gpu, alg, extra):
    exe = os.path.join(PKG, "bin", "native_mi355")
    out = subprocess.run([exe, "-a", alg, "-r", "65536", "-s", "262144"] + extra, capture_output=True, text=True,
                         timeout=120, check=True).stdout
    assert "Result tuples : 262144" in out and "Matches = 262144" in out and f"Running {alg}" in out
    if "-m" in extra:
        assert "Materialized 262144 tuples" in out
    r_passes = 0 if "--sort-r" in extra else 2
    s_passes = 0 if "--sort-s" in extra else 2
    assert f"{r_passes} + {s_passes} radix-sort passes" in out
    lines = PSM_LINES if alg == "PSM" else RADIX_LINES
    pos = [out.index(t) for t in lines]  # the reference's print_timing lines, in its order
    assert pos == sorted(pos)
    throughput, phases = parse_teebench_output(out)
    assert throughput > 0
    want = {"total", "partition", "join_total"} | (set() if alg == "PSM" else {"partition_1", "partition_2", "build",
                                                                               "probe"})
    assert set(phases) == want
    assert phases["total"] > 0 and phases["join_total"] > 0
    assert (phases["partition"] > 0) == (r_passes + s_passes > 0)
    assert phases["partition"] + phases["join_total"] <= phases["total"] + 2
    for k in want - {"total", "partition", "join_total"}:
        assert phases[k] == 0


@pytest.mark.parametrize("alg", ["RHO", "PHT"])
def test_native_driver_sort_flags_hold_for_other_joins(gpu, alg):
    exe = os.path.join(PKG, "bin", "native_mi355")
    out = subprocess.run([exe, "-a", alg, "-r", "65536", "-s", "262144", "--sort-r", "--sort-s"],
                         capture_output=True, text=True, timeout=120, check=True).stdout
    assert "Matches = 262144" in out


# ---------------------------------------------------------------------- neighbours
def test_neighbours_are_undisturbed(sgx, orc, gpu):
    rng = np.random.default_rng(17)
    R = rel(rng.integers(0, 3000, 20_000))
    S = rel(rng.integers(0, 3000, 30_000))
    exp = orc.count_join_sort(R, S)
    assert sgx.npo_join(R, len(R), S, len(S)).matches == exp
    before = sgx.last_npo_stats()
    assert smj(sgx, R, S).matches == exp
    assert sgx.last_npo_stats() == before
    assert sgx.rho_join(R, len(R), S, len(S)).matches == exp
    assert sgx.npo_join(R, len(R), S, len(S)).matches == exp
    assert sgx.rho_join(R, len(R), S, len(S), algorithm="RHT").matches == exp
    sgx.release_workspace()
    assert smj(sgx, R, S).matches == exp
    assert sgx.rho_join(R, len(R), S, len(S)).matches == exp
