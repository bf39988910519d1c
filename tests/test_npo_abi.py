"""The no-partitioning join's boundary (PHT family) without a GPU: exported symbols,
header, ctypes mirrors and the argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libsgxamd.so")

# npj/no_partitioning_hash_join.hpp:6-16, mangled by g++ from those declarations
PHT_SYMBOLS = {
    "PHT": "_Z3PHTPK7table_tS1_PK12joinconfig_t",
    "PHT_no_overflow": "_Z15PHT_no_overflowPK7table_tS1_PK12joinconfig_t",
    "PHT_unrolled": "_Z12PHT_unrolledPK7table_tS1_PK12joinconfig_t",
    "PHT_overflow": "_Z12PHT_overflowPK7table_tS1_PK12joinconfig_t",
}
C_SYMBOLS = ["mi355_npo_join", "mi355_npo_join_ex", "mi355_last_npo_stats"]


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_pht_cxx_symbols_exported():
    exp = exported()
    for name, mangled in PHT_SYMBOLS.items():
        assert mangled in exp, name
    # the two NPO_* table names have no C++ symbol (sgxamd/joins.hpp)
    assert not [s for s in exp if "NPO_" in s]


def test_pht_mangled_names_come_from_the_header(tmp_path):
    """The declarations in sgxamd/joins.hpp, defined by a g++-compiled file, give the
    symbols the library exports."""
    src = tmp_path / "decl.cpp"
    body = "".join(f"result_t *{n}(const table_t *, const table_t *, const joinconfig_t *) {{ return nullptr; }}\n"
                   for n in PHT_SYMBOLS)
    src.write_text('#include "sgxamd/joins.hpp"\n' + body)
    obj = tmp_path / "decl.o"
    subprocess.run(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)],
                   check=True)
    out = subprocess.run(["nm", "--defined-only", str(obj)], capture_output=True, text=True, check=True).stdout
    got = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert got == set(PHT_SYMBOLS.values())


def test_npo_c_symbols_exported_and_bound(sgx):
    exp = exported()
    for name in C_SYMBOLS:
        assert name in exp, name
        assert name in sgx.SIGNATURES, name
        assert getattr(sgx.lib, name).argtypes == sgx.SIGNATURES[name][1]
    assert "PHT" not in sgx.ALGORITHMS  # that dict feeds mi355_rho_opts.algorithm


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    use = ('#include "sgxamd/rho.h"\n'
           "int main(void) {\n"
           "  mi355_npo_opts o = {0};\n  mi355_npo_stats s = {0};\n"
           "  o.bucket_bits = MI355_ALGO_PHT;\n"
           "  return (int)(s.matches + s.num_buckets + s.overflow_nodes + s.max_chain + s.table_bytes) + o.timing +\n"
           "         mi355_npo_join_ex(0, 0, 0, 0, &o, &s) + mi355_npo_join(0, 0, 0, 0) + mi355_last_npo_stats(&s);\n}\n")
    c = tmp_path / "t.c"
    c.write_text(use)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text(use.replace("{0}", "{}"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(cpp),
                    "-o", str(tmp_path / "cpp.o")], check=True)


def test_npo_structs_match_ctypes(sgx, tmp_path):
    structs = {"mi355_npo_opts": sgx.npo_opts, "mi355_npo_stats": sgx.npo_stats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sgxamd/rho.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "npo_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "npo_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in out if line}
    for cname, py in structs.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in sgx.npo_opts._fields_] == ["bucket_bits", "materialize", "timing", "stream", "out",
                                                     "out_capacity"]


def test_npo_without_gpu_fails_loudly(sgx):
    if sgx.device_count() > 0:
        return
    R = np.zeros(16, dtype=np.uint64)
    for call in (lambda: sgx.npo_join(R, 16, R, 16), lambda: sgx.npo_join_tables(R, 16, R, 16)):
        try:
            call()
        except sgx.Mi355Error as e:
            assert e.code == sgx.MI355_ERR_NO_DEVICE
        else:
            raise AssertionError("the no-partitioning join ran without a GPU")


def test_npo_rejects_bad_arguments_before_device_work(sgx):
    """Null relations with non-zero sizes, a null out with a capacity, bucket_bits out of
    range and a null table are MI355_ERR_INVALID on any host: the checks come before the
    device is looked up."""
    R = np.zeros(16, dtype=np.uint64)
    out = np.zeros((4, 3), dtype=np.uint32)
    bad = [
        lambda: sgx.npo_join(None, 16, R, 16),
        lambda: sgx.npo_join(R, 16, None, 16),
        lambda: sgx.npo_join(None, 1, None, 1, out=out, out_capacity=4),
        lambda: sgx.npo_join(R, 16, R, 16, bucket_bits=32),
        lambda: sgx.npo_join(R, 16, R, 16, bucket_bits=-1),
    ]
    for i, call in enumerate(bad):
        try:
            call()
        except sgx.Mi355Error as e:
            assert e.code == sgx.MI355_ERR_INVALID, i
        else:
            raise AssertionError(i)
    o = sgx.npo_opts(0, 1, 0, None, None, 8)  # materialize, out NULL, capacity 8
    assert sgx.lib.mi355_npo_join_ex(sgx.ptr(R), 16, sgx.ptr(R), 16, C.byref(o), None) == sgx.MI355_ERR_INVALID
    assert sgx.lib.mi355_npo_join(None, None, None, None) == sgx.MI355_ERR_INVALID
    assert sgx.lib.mi355_last_npo_stats(None) == sgx.MI355_ERR_INVALID
