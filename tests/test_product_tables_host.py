"""CPU: the index tables of a product POVM (quantpy_amd/csrc/qt_product_tables.h), which qt_set_povm_product uploads as
they come.  tests/host/product_tables_host.cpp is a program of its own: it builds the tables for n = 1..5 and the edges of
the admitted range, checks their sizes against the kernels' fwd_ints / bwd_ints, runs the stages through them as
Small::stage_value does against a plain Kronecker evaluation, checks the paired `last` table and the table image, and
the refusals.  Run once as built and once under AddressSanitizer and UBSan, as an executable: nothing is loaded into
Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "product_tables_host.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert " 0 failed" in res.stdout, res.stdout[-2000:]
    return res


def test_product_tables(tmp_path):
    _build_and_run(tmp_path, "product_tables", ["-O2"])


def test_product_tables_under_asan_and_ubsan(tmp_path):
    asan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("g++ has no libasan here")
    res = _build_and_run(tmp_path, "product_tables_san", SAN)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
