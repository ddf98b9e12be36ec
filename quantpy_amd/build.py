"""Build libqtomo.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB = os.path.join(LIB_DIR, "libqtomo.so")


# max-ilp: hipcc's default scheduler optimises for occupancy; these kernels run one to five waves per SIMD
# with registers to spare, and the ILP strategy (loads hoisted, independent chains interleaved) measured
# 4-5 % faster on every n = 3 kernel (profiles/round1_v11_*).
SCHED_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# A kernel's leading pointer and scalar arguments, up to its first struct, arrive in SGPRs at wave launch instead of
# through an s_load from the argument segment (a cold read in front of every address).  The n <= 3 MLE kernels lead with
# what their first loads need (csrc/qt_args.h: mle_front).  A kernel that leads with a struct preloads nothing.
PRELOAD_FLAGS = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
FLAGS = SCHED_FLAGS + PRELOAD_FLAGS
# qtomo.hip is the library; qt_lp_pieces.hip holds the kernel of the test entry qt_lp_pieces, apart from the kernels it inspects
SOURCES = [os.path.join(CSRC, "qtomo.hip"), os.path.join(CSRC, "qt_lp_pieces.hip")]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _source_hash():
    """SHA-256 over the HIP sources, the public header and the compiler flags."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + [os.path.join(os.path.dirname(_HERE), "include", "qtomo.h")]
    for path in srcs:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _stale():
    """True unless lib/libqtomo.so was built from exactly the sources in the tree (hash, not mtime: a shipped
    library newer than edited-and-reverted or freshly checked-out sources must not be trusted on its date)."""
    if not os.path.exists(LIB) or not os.path.exists(LIB + ".srchash"):
        return True
    with open(LIB + ".srchash") as fh:
        return fh.read().strip() != _source_hash()


def build_profile_library(verbose=False):
    """Development aid: the same sources with -DQT_PHASE_TIMING -> lib/libqtomo_prof.so (phase stamps
    inside the kernels; loaded only when QTOMO_LIB points at it, see scripts/phase_timing.py)."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "libqtomo_prof.so")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-DQT_PHASE_TIMING", *FLAGS,
           "-o", out, *SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -shared -fPIC csrc/qtomo.hip csrc/qt_lp_pieces.hip -> lib/libqtomo.so"""
    if not force and not _stale():
        return LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", *FLAGS,
           "-o", LIB + ".tmp", *SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    with open(LIB + ".srchash", "w") as fh:
        fh.write(_source_hash() + "\n")
    return LIB
