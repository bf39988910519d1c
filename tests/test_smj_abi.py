"""The sort-merge join's boundary (MWAY / PSM / RSM, mi355_sort_rows) without a GPU:
exported symbols, header, ctypes mirrors and the argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libsgxamd.so")

# mway/sortmergejoin_multiway.h:40-41, psm/parallel_sortmerge_join.h:16,
# radix/radix_sortmerge_join.hpp:4, mangled by g++ from those declarations
SMJ_SYMBOLS = {
    "MWAY": "_Z4MWAYPK7table_tS1_PK12joinconfig_t",
    "PSM": "_Z3PSMPK7table_tS1_PK12joinconfig_t",
    "RSM": "_Z3RSMPK7table_tS1_PK12joinconfig_t",
}
C_SYMBOLS = ["mi355_smj_join", "mi355_smj_join_ex", "mi355_last_smj_stats", "mi355_sort_rows"]


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_smj_cxx_symbols_exported():
    exp = exported()
    for name, mangled in SMJ_SYMBOLS.items():
        assert mangled in exp, name


def test_smj_mangled_names_come_from_the_header(tmp_path):
    """The declarations in sgxamd/joins.hpp, defined by a g++-compiled file, give the
    symbols the library exports."""
    src = tmp_path / "decl.cpp"
    body = "".join(f"result_t *{n}(const table_t *, const table_t *, const joinconfig_t *) {{ return nullptr; }}\n"
                   for n in SMJ_SYMBOLS)
    src.write_text('#include "sgxamd/joins.hpp"\n' + body)
    obj = tmp_path / "decl.o"
    subprocess.run(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)],
                   check=True)
    out = subprocess.run(["nm", "--defined-only", str(obj)], capture_output=True, text=True, check=True).stdout
    got = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert got == set(SMJ_SYMBOLS.values())


def test_smj_c_symbols_exported_and_bound(sgx):
    exp = exported()
    for name in C_SYMBOLS:
        assert name in exp, name
        assert name in sgx.SIGNATURES, name
        assert getattr(sgx.lib, name).argtypes == sgx.SIGNATURES[name][1]
    assert sgx.ALGORITHMS == {"RHO": 0, "RHT": 1}  # that dict feeds mi355_rho_opts.algorithm


def test_header_compiles_as_c11_and_cxx17(tmp_path):
    use = ('#include "sgxamd/rho.h"\n'
           "int main(void) {\n"
           "  mi355_smj_opts o = {0};\n  mi355_smj_stats s = {0};\n  uint32_t p = 0;\n"
           "  o.r_sorted = MI355_ALGO_SMJ; o.s_sorted = 0; o.materialize = 0; o.out = 0; o.out_capacity = 0; o.stream = 0;\n"
           "  return (int)(s.matches + s.sort_passes_r + s.sort_passes_s + s.elem_bytes + s.sort_tile + s.merge_tile +\n"
           "               s.reserved0) + (int)(s.ms_h2d + s.ms_sort_r + s.ms_sort_s + s.ms_merge + s.ms_total) + o.timing +\n"
           "         mi355_smj_join_ex(0, 0, 0, 0, &o, &s) + mi355_smj_join(0, 0, 0, 0) + mi355_last_smj_stats(&s) +\n"
           "         mi355_sort_rows(0, 0, 0, &p, 0);\n}\n")
    c = tmp_path / "t.c"
    c.write_text(use)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text(use.replace("{0}", "{}"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(cpp),
                    "-o", str(tmp_path / "cpp.o")], check=True)


def test_smj_structs_match_ctypes(sgx, tmp_path):
    structs = {"mi355_smj_opts": sgx.smj_opts, "mi355_smj_stats": sgx.smj_stats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sgxamd/rho.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "smj_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "smj_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in out if line}
    for cname, py in structs.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in sgx.smj_opts._fields_] == ["r_sorted", "s_sorted", "materialize", "timing", "stream", "out",
                                                     "out_capacity"]
    assert [f for f, _ in sgx.smj_stats._fields_] == ["matches", "sort_passes_r", "sort_passes_s", "elem_bytes",
                                                      "sort_tile", "merge_tile", "reserved0", "ms_h2d", "ms_sort_r",
                                                      "ms_sort_s", "ms_merge", "ms_total"]


def test_smj_without_gpu_fails_loudly(sgx):
    if sgx.device_count() > 0:
        return
    R = np.zeros(16, dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint64)
    for call in (lambda: sgx.smj_join(R, 16, R, 16), lambda: sgx.smj_join_tables(R, 16, R, 16),
                 lambda: sgx.sort_rows(R, 16, out)):
        try:
            call()
        except sgx.Mi355Error as e:
            assert e.code == sgx.MI355_ERR_NO_DEVICE
        else:
            raise AssertionError("the sort-merge join ran without a GPU")


def test_smj_rejects_bad_arguments_before_device_work(sgx):
    """A null relation with a non-zero size, a null out with a capacity, an in-place sort
    and a null table are MI355_ERR_INVALID on any host: the checks come before the device
    is looked up."""
    R = np.zeros(16, dtype=np.uint64)
    out = np.zeros((4, 3), dtype=np.uint32)
    bad = [
        lambda: sgx.smj_join(None, 16, R, 16),
        lambda: sgx.smj_join(R, 16, None, 16),
        lambda: sgx.smj_join(None, 1, None, 1, out=out, out_capacity=4),
        lambda: sgx.smj_join(R, (1 << 31) + 1, R, 16),
        lambda: sgx.sort_rows(None, 16, R),
        lambda: sgx.sort_rows(R, 16, None),
        lambda: sgx.sort_rows(R, 16, R),
    ]
    for i, call in enumerate(bad):
        try:
            call()
        except sgx.Mi355Error as e:
            assert e.code == sgx.MI355_ERR_INVALID, i
        else:
            raise AssertionError(i)
    o = sgx.smj_opts(0, 0, 1, 0, None, None, 8)  # materialize, out NULL, capacity 8
    assert sgx.lib.mi355_smj_join_ex(sgx.ptr(R), 16, sgx.ptr(R), 16, C.byref(o), None) == sgx.MI355_ERR_INVALID
    assert sgx.lib.mi355_smj_join(None, None, None, None) == sgx.MI355_ERR_INVALID
    assert sgx.lib.mi355_last_smj_stats(None) == sgx.MI355_ERR_INVALID
    assert sgx.sort_rows(None, 0, None) == 0  # an empty sort touches no device
