"""CPU, compiler only: how the headers of quantpy_amd/csrc compose.

Every header compiles as the only include of a translation unit, so none leans on what another happened to include in
front of it; and qt_sampler.h, whose arithmetic must not be contracted, keeps that to its own function bodies: a kernel
defined behind it still gets its fused multiply-adds (a file-scope `#pragma clang fp contract(off)` holds to the end of
the translation unit, whatever namespace it stands in)."""
import glob
import os
import re
import subprocess

import pytest
from conftest import ROOT

CSRC = os.path.join(ROOT, "quantpy_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))


@pytest.fixture(scope="module")
def hipcc():
    from quantpy_amd.build import _hipcc

    try:
        return _hipcc()
    except RuntimeError:
        pytest.skip("no hipcc here")


def test_the_headers_were_found():  # (an empty parametrisation below would pass in silence)
    assert "qt_wave.h" in HEADERS and "qt_sampler.h" in HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(hipcc, header, tmp_path):
    tu = tmp_path / "tu.hip"
    tu.write_text(f'#include "{header}"\n')
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _function(asm, name):
    """The instructions of the function whose mangled name contains `name`."""
    m = re.search(r"^(_Z\w*" + name + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.M | re.S)
    assert m, f"{name} not in the assembly"
    return [ln.split()[0] for ln in m.group(2).split("\n") if ln.strip() and not ln.lstrip().startswith((";", "."))]


def test_sampler_keeps_its_no_contraction_to_itself(hipcc, tmp_path):
    tu = tmp_path / "leak.hip"
    tu.write_text('#include "qt_sampler.h"\n'
                  "__global__ void probe(double* x, double a, double b) { x[0] = a * b + x[0]; }\n"
                  "__global__ void probe_u53(double* x, uint32_t a, uint32_t b) { x[0] = qt_sampler::u53_words(a, b); }\n")
    out = tmp_path / "leak.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "-S", "--cuda-device-only", "-I", CSRC,
                           "-o", str(out), str(tu)])
    asm = out.read_text()
    fused = ("v_fma_f64", "v_fmac_f64")
    # behind the header: contracted as everywhere else
    ops = _function(asm, "5probePd")
    assert any(op.startswith(fused) for op in ops), ops
    # inside the header's own function, inlined into a kernel: a product, rounded, then a sum
    ops = _function(asm, "9probe_u53")
    assert not any(op.startswith(fused) for op in ops), ops
    # (the product a * 2^26 is exact and may come out as v_ldexp_f64; contracted, it is v_fmac_f64 with that constant)
    mul = [i for i, op in enumerate(ops) if op.startswith(("v_mul_f64", "v_ldexp_f64"))]
    add = [i for i, op in enumerate(ops) if op.startswith("v_add_f64")]
    assert mul and add and mul[0] < add[0], ops
