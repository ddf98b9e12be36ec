"""Cases, references and bounds for the primitives of the three LP kernels as qt_lp_pieces hands them out
(csrc/qt_lp_pieces.hip): the normal matrix H = A^T diag(w) A (bordered with the phase-1 column -1 when p1), its Cholesky
factor L, u = A^T vm, ax = A vn and the solve (L L^T)^-1 vn.  Shared by test_lp_pieces_host.py, which runs every
assertion on a NumPy float64 model of the kernel (no GPU), and test_gpu_lp_pieces.py, which runs them on the kernels.

References are NumPy in np.longdouble (64-bit mantissa on x86).  Every bound is an a-priori rounding bound with
gamma_k = k u / (1 - k u), u = 2^-53; it holds for any summation order, with or without FMA, and none is tuned to a kernel:

    normal   |H - H_ref|[i, j] <= gamma_{M+3} sum_k |w_k A_ki A_kj|                    (i >= j, border terms included)
    u, ax    the same form with gamma_{M+3} over |A|^T |vm| and gamma_{N+3} over |A| |vn|
    factor   against the kernel's own H bits: |L L^T - H|[i, j] <= gamma_{n+2} (|L| |L|^T)[i, j] on the lower triangle;
             a replaced pivot's diagonal entry is exempt, there L[k, k] == sqrt(H[k, k]) bit for bit, and the replaced
             positions are those of lp_model.cholesky_replacing on the kernel's H
    solved   against the kernel's own L: |L L^T x - v|_i <= gamma_{3n+2} (|L| |L|^T |x|)_i, and against the longdouble
             solution of the reference H within cond_2(H) gamma_{3n+M} (relative, 2-norm)

Above n = FULL_FROM a longdouble product of the whole triangle takes too long (17 s at n = 1024): there the whole triangle
is compared with float64 BLAS at twice the bound (both sides round) and a fixed-seed sample of SAMPLE entries -- the
diagonal's ends, rows and columns 127 / 128, 255 / 256, 895 / 896, 1023 and the border row among them -- in longdouble
at the bound itself; the model factorisation that names the replaced pivots runs in float64, and the comparison with
a longdouble solution is left out.

Inputs: A Gaussian; where M < 2 N its leading N x N block gets 2 sqrt(N) I added (a square Gaussian matrix has pivots
within reach of the safeguard's threshold); w = 10^U(-2, 2); vm, vn Gaussian.  The safeguard cases repeat a column
exactly ('repeat': its pivot is rounding noise of either sign), or up to NEAR times a Gaussian column ('near': a pivot
that is positive by construction and still far below the threshold), zero a column, or put a NaN into w.  A case that expects no replaced pivot, or
exactly one, keeps every other pivot ratio of the model outside [1e-13, 1e-9] (`check_pivot_gap`, asserted by the host
test for every such case), so the kernel's rounding cannot move a pivot across its threshold (1e-11 or 1e-12).
"""
import functools
from collections import namedtuple

import lp_model
import numpy as np

assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble has no 64-bit mantissa here: the references need one"

LD = np.longdouble
U = 2.0 ** -53
FULL_FROM = 401  # n from which the reference of a triangle is sampled
SAMPLE = 4096
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)
SMALL, LARGE, XL = 0, 1, 2
KERNEL_NAME = {SMALL: "small", LARGE: "large", XL: "xl"}
MAX_N = {SMALL: 64, LARGE: 255, XL: 1023}
PIVOT = {0: {SMALL: 0.0, LARGE: lp_model.LARGE_PIVOT, XL: lp_model.LARGE_PIVOT}, 1: {k: 1e-12 for k in (SMALL, LARGE, XL)}}


def gamma(k):
    return k * U / (1.0 - k * U)


# kind: 'random'; 'repeat' (column repeat_of(N)[1] is column repeat_of(N)[0]); 'near' (the same plus NEAR times a
# Gaussian column: the pivot is positive, about 1e-14 of its diagonal entry, above the rounding noise of a float64 H
# (some 5e-16) and a thousandth of the threshold -- a safeguard that only catches non-positive pivots keeps it); 'zero' (column
# zero_col_of(N) is 0); 'nan_w' (one weight NaN)
NEAR = 3e-7
Shape = namedtuple("Shape", "M N p1 mode kind")


def shape_id(s):
    return "%s-M%d-N%d-p%d-mode%d" % (s.kind, s.M, s.N, s.p1, s.mode)


# ---- the shapes ------------------------------------------------------------------------------------------------------
# XL: N at the 32-column panel (1, 31, 32, 33), the 128-block of xl_syrk (127, 128, 129), the 256-thread stride of the
# vector loops (255, 256, 257), a fourth block of one column (385); M = N, M < 16, M mod 16 in {0, 1, 15}, M mod 4 != 0
_XL_MN = [(1, 1), (7, 1), (31, 31), (48, 31), (32, 32), (33, 32), (33, 33), (47, 33), (127, 127), (130, 127), (128, 128),
          (145, 128), (129, 129), (261, 129), (255, 255), (272, 255), (256, 256), (271, 256), (257, 257), (300, 257),
          (385, 385), (402, 385)]
XL_SHAPES = [Shape(M, N, p1, 0, "random") for M, N in _XL_MN for p1 in (0, 1)]
XL_FULL_SHAPES = [Shape(1100, 1023, 1, 0, "random"), Shape(7776, 1023, 1, 0, "random")]
LARGE_SHAPES = [Shape(M, N, p1, 0, "random") for N in (15, 64, 65, 96, 97, 128, 129, 255) for M in (N, 2 * N + 3)
                for p1 in (0, 1)]
# (the small kernel's plain Cholesky has no answer of its own to a singular H, so its list has M = N + 1 for M = N: with
# the border, M = N rows give n = N + 1 columns rank N, see expected_replaced)
SMALL_SHAPES = [Shape(M, N, p1, 0, "random") for N in (1, 2, 15, 63, 64) for M in (N + 1, 3 * N + 1) for p1 in (0, 1)]
RANK_TEST_SHAPES = [Shape(2 * N + 3, N, 0, 1, "random") for N in (64, 129, 300)]  # mode 1 on a full-rank A
SAFEGUARD_N = {LARGE: (129,), XL: (129, 300)}


def kernels_of(s):
    """The kernels a shape of the lists above runs on: its own list's, and for the small and large lists every larger
    kernel too (they must agree)."""
    return [k for k in (SMALL, LARGE, XL) if s.N <= MAX_N[k] and (k != SMALL or s in SMALL_SHAPES or s.mode == 1)]


def reference_cases():
    """(kernel, shape) of every comparison with the reference."""
    out = [(XL, s) for s in XL_SHAPES + XL_FULL_SHAPES]
    out += [(k, s) for s in LARGE_SHAPES for k in (LARGE, XL)]
    out += [(k, s) for s in SMALL_SHAPES for k in (SMALL, LARGE, XL)]
    out += [(k, s) for s in RANK_TEST_SHAPES for k in kernels_of(s)]
    return out


def agreement_shapes():
    return SMALL_SHAPES + LARGE_SHAPES


def safeguard_cases():
    """(kernel, shape, expected ok, expected replaced positions or None)."""
    out = []
    for k, sizes in SAFEGUARD_N.items():
        for N in sizes:
            M = 2 * N + 3
            for p1 in (0, 1):
                out.append((k, Shape(M, N, p1, 0, "repeat"), 1, (repeat_of(N)[1],)))
                out.append((k, Shape(M, N, p1, 0, "near"), 1, (repeat_of(N)[1],)))
                out.append((k, Shape(M, N, p1, 0, "zero"), 0, None))
                out.append((k, Shape(M, N, p1, 0, "nan_w"), 0, None))
            out.append((k, Shape(M, N, 0, 1, "repeat"), 0, None))
            out.append((k, Shape(M, N, 0, 1, "near"), 0, None))
            out.append((k, Shape(M, N, 0, 1, "zero"), 0, None))
            out.append((k, Shape(M, N, 0, 1, "nan_w"), 0, None))
    return out


def expected_replaced(s):
    """The pivots a 'random' shape replaces in mode 0: none -- but M = N rows with the border are n = N + 1 columns of
    rank N, whose last pivot is rounding noise of either sign, far below the threshold: exactly that one."""
    return (s.N,) if (s.kind == "random" and s.mode == 0 and s.p1 and s.M == s.N) else ()


def repeat_of(N):
    """(the column that is copied, the column that is its copy): in different 32-column panels where N allows."""
    return (N // 5, N - 1 - N // 7) if N > 2 else (0, N - 1)


def zero_col_of(N):
    return (2 * N) // 3


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(M, N, kind):
    rng = np.random.default_rng([M, N, {"random": 0, "repeat": 1, "zero": 2, "nan_w": 3, "near": 4}[kind]])
    A = rng.standard_normal((M, N))
    if M < 2 * N:
        A[:N] += 2.0 * np.sqrt(N) * np.eye(N)
    w = 10.0 ** rng.uniform(-2.0, 2.0, M)
    vm = rng.standard_normal(M)
    vn = rng.standard_normal(N + 1)
    if kind == "repeat":
        a, b = repeat_of(N)
        A[:, b] = A[:, a]
    elif kind == "near":
        a, b = repeat_of(N)
        A[:, b] = A[:, a] + NEAR * rng.standard_normal(M)
    elif kind == "zero":
        A[:, zero_col_of(N)] = 0.0
    elif kind == "nan_w":
        w[M // 2] = np.nan
    for v in (A, w, vm, vn):
        v.setflags(write=False)
    return A, w, vm, vn


def inputs(s):
    """-> A (M, N), w (M,), vm (M,), vn (n,): the same for every kernel, and for p1 = 0 / 1 up to vn's last entry."""
    A, w, vm, vn = _inputs(s.M, s.N, s.kind)
    return A, w, vm, vn[:s.N + s.p1]


def colsum_sign(s):
    """colsum hands out u[N] = +sum(vm), not the border column's -sum(vm): [A, -1]^T vm with the last sign turned."""
    sign = np.ones(s.N + s.p1)
    if s.p1:
        sign[s.N] = -1.0
    return sign


def bordered(A, p1, dtype=np.float64):
    A = A.astype(dtype)
    return np.hstack([A, -np.ones((A.shape[0], 1), dtype=dtype)]) if p1 else A


def model(s):
    """What a correct float64 implementation hands out: the stand-in for the kernel in the host test (BLAS products,
    lp_model.cholesky_replacing, np.linalg.solve); the layout and the fill of Engine.lp_pieces."""
    A, w, vm, vn = inputs(s)
    Af = bordered(A, s.p1)
    n = Af.shape[1]
    fill = np.full((n, n), np.nan).view(np.uint64)
    fill[:] = POISON
    H = Af.T @ (w[:, None] * Af)
    out = {"normal": np.where(np.tri(n, dtype=bool), H, fill.view(np.float64)), "u": colsum_sign(s) * (Af.T @ vm),
           "ax": A @ vn[:s.N]}
    out["factor"] = fill.view(np.float64).copy()
    out["solved"] = fill.view(np.float64)[0].copy()
    try:
        trace = []
        with np.errstate(all="ignore"):
            L = lp_model.cholesky_replacing(np.tril(H) + np.tril(H, -1).T, PIVOT[s.mode][LARGE], trace)[0]
        good = np.all(np.isfinite(L)) and not (s.mode == 1 and any(r for _, r in trace))
    except np.linalg.LinAlgError:
        good = False
    out["ok"] = int(good)
    if good:
        out["factor"] = np.where(np.tri(n, dtype=bool), L, fill.view(np.float64))
        out["solved"] = np.linalg.solve(L.T, np.linalg.solve(L, vn))
    return out


# ---- references ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sample(n, p1):
    """Fixed-seed (i, j), i >= j, of the sampled comparison, SAMPLE of them: every pair of the named rows / columns,
    spans along each of them, the diagonal, every seventh entry of the border row, the rest drawn uniformly."""
    marks = [k for k in (0, 31, 32, 127, 128, 255, 256, 895, 896, 1023, n - 1) if k < n]
    pairs = {(max(a, b), min(a, b)) for a in marks for b in marks} | {(k, k) for k in range(n)}
    for m in marks:  # along every named row and column: every 37th entry, and the neighbours of the other seams
        along = set(range(0, n, 37)) | {k + d for k in marks for d in (-1, 1) if 0 <= k + d < n}
        pairs |= {(max(m, k), min(m, k)) for k in along}
    if p1:
        pairs |= {(n - 1, j) for j in range(0, n, 7)}
    assert len(pairs) < SAMPLE
    rng = np.random.default_rng([n, SAMPLE])
    while len(pairs) < SAMPLE:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        pairs.add((max(a, b), min(a, b)))
    ij = np.array(sorted(pairs))
    return ij[:, 0], ij[:, 1]


@functools.lru_cache(maxsize=4)
def _normal_reference(M, N, kind):
    """The bordered (p1 = 1) reference of H and of its bound's sum; p1 = 0 is its leading block.  -> a dict: whole
    (longdouble H_ref, S) below FULL_FROM, else the float64 product, its S and the longdouble sample."""
    A, w, _, _ = _inputs(M, N, kind)
    n = N + 1
    if n < FULL_FROM:
        Af = bordered(A, 1, LD)
        wl = w.astype(LD)
        return {"H": Af.T @ (wl[:, None] * Af), "S": np.abs(Af).T @ (np.abs(wl)[:, None] * np.abs(Af))}
    Af = bordered(A, 1)
    out = {"H64": Af.T @ (w[:, None] * Af), "S64": np.abs(Af).T @ (np.abs(w)[:, None] * np.abs(Af))}
    i, j = _sample(n, 1)
    Al, wl = Af.astype(LD), w.astype(LD)
    Hs, Ss = np.empty(i.size, dtype=LD), np.empty(i.size, dtype=LD)
    for k in range(0, i.size, 256):  # in blocks: M x SAMPLE longdoubles are 0.5 GB at M = 7776
        P = wl[:, None] * Al[:, i[k:k + 256]] * Al[:, j[k:k + 256]]
        Hs[k:k + 256], Ss[k:k + 256] = P.sum(axis=0), np.abs(P).sum(axis=0)
    out.update(i=i, j=j, Hs=Hs, Ss=Ss)
    return out


@functools.lru_cache(maxsize=4)
def _solution_reference(M, N, kind, p1):
    """-> (the longdouble solution of H_ref x = vn, cond_2(H_ref)), n < FULL_FROM."""
    n = N + p1
    Href = _normal_reference(M, N, kind)["H"][:n, :n]
    Lref, _ = pivot_trace(Href, 0.0)
    return _ld_solve(Lref, _inputs(M, N, kind)[3][:n]), float(np.linalg.cond(Href.astype(np.float64)))


def _worst(err, bound):
    """max err / bound over the entries (0 / 0 counts as 0; anything over a zero bound as inf)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def _sym(lower):
    """The symmetric matrix of a lower triangle whose upper part holds the fill."""
    t = np.tril(lower.astype(LD))
    return t + np.tril(t, -1).T


def _ld_solve(L, v):
    """(L L^T)^-1 v in L's precision, column sweeps."""
    x = v.astype(L.dtype).copy()
    n = x.size
    for k in range(n):
        x[k] /= L[k, k]
        x[k + 1:] -= L[k + 1:, k] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] /= L[k, k]
        x[:k] -= L[k, :k] * x[k]
    return x


def pivot_trace(H, rel):
    """lp_model.cholesky_replacing on H (in H's precision) -> (L or None on a breakdown, [(ratio, replaced), ...])."""
    trace = []
    try:
        with np.errstate(all="ignore"):
            L = lp_model.cholesky_replacing(H, rel, trace)[0]
    except np.linalg.LinAlgError:
        L = None
    return L, trace


def model_precision(n):
    return LD if n < FULL_FROM else np.float64


def check_pivot_gap(s, expected_replaced=()):
    """No pivot ratio of the model on the reference H lies in [1e-13, 1e-9], the expected replacements apart (theirs
    are below 1e-13).  -> the smallest other ratio."""
    ref = _normal_reference(s.M, s.N, s.kind)
    n = s.N + s.p1
    H = (ref["H"] if "H" in ref else ref["H64"])[:n, :n]
    _, trace = pivot_trace(H, lp_model.LARGE_PIVOT)
    assert len(trace) == n
    ratios = np.array([r for r, _ in trace])
    others = np.delete(ratios, list(expected_replaced))
    assert np.all(ratios[list(expected_replaced)] < 1e-13), ratios[list(expected_replaced)]
    if s.kind == "near":  # positive, and clear of the rounding noise of a float64 H (about n u)
        assert np.all(ratios[list(expected_replaced)] > 5e-15), ratios[list(expected_replaced)]
    assert np.all(others >= 1e-9), others.min()
    return float(others.min())


def check_poison_and_shape(s, out):
    """No NaN in a defined output; the strict upper triangles still hold the fill; `solved` is written iff ok."""
    n = s.N + s.p1
    low = np.tri(n, dtype=bool)
    for name in ("normal", "factor"):
        assert out[name].shape == (n, n)
        assert np.all(out[name].view(np.uint64)[~low] == POISON), name + ": the upper triangle was written"
    assert not np.isnan(out["u"]).any() and not np.isnan(out["ax"]).any()
    assert out["ok"] in (0, 1)
    if s.kind != "nan_w":
        assert not np.isnan(out["normal"][low]).any()
    if out["ok"]:
        assert not np.isnan(out["factor"][low]).any() and not np.isnan(out["solved"]).any()
    else:
        assert np.all(out["solved"].view(np.uint64) == POISON)


def check_products(s, out, tag=""):
    """normal, u and ax against the reference.  -> {name: largest error / bound}."""
    A, w, vm, vn = inputs(s)
    M, N, n = s.M, s.N, s.N + s.p1
    low = np.tri(n, dtype=bool)
    ref = _normal_reference(s.M, s.N, s.kind)
    worst = {}
    g = gamma(M + 3)
    if "H" in ref:
        err = np.abs(out["normal"].astype(LD) - ref["H"][:n, :n])[low]
        worst["normal"] = _worst(err, g * ref["S"][:n, :n][low])
    else:
        err = np.abs(out["normal"] - ref["H64"][:n, :n])[low]
        worst["normal (float64 BLAS, twice the bound)"] = _worst(err, 2.0 * g * ref["S64"][:n, :n][low])
        keep = ref["i"] < n
        i, j = ref["i"][keep], ref["j"][keep]
        err = np.abs(out["normal"][i, j].astype(LD) - ref["Hs"][keep])
        worst["normal"] = _worst(err, g * ref["Ss"][keep])
    Al, Afl = A.astype(LD), bordered(A, s.p1, LD)
    worst["u"] = _worst(np.abs(out["u"].astype(LD) - colsum_sign(s) * (Afl.T @ vm.astype(LD))),
                        g * (np.abs(Afl).T @ np.abs(vm).astype(LD)))
    worst["ax"] = _worst(np.abs(out["ax"].astype(LD) - Al @ vn[:N].astype(LD)),
                         gamma(N + 3) * (np.abs(Al) @ np.abs(vn[:N]).astype(LD)))
    print("LPPIECES", tag, shape_id(s), "error / bound:", {k: "%.3g" % v for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
    return worst


def check_factor(s, out, rel, replaced=()):
    """factor against the kernel's own normal: the backward error, the replaced pivots and their set.
    -> {name: largest error / bound}."""
    n = s.N + s.p1
    low = np.tri(n, dtype=bool)
    assert out["ok"] == 1
    dt = model_precision(n)
    Hk = _sym(out["normal"]).astype(dt)
    L = np.tril(out["factor"]).astype(dt)
    _, trace = pivot_trace(Hk, rel)
    assert len(trace) == n, "the model breaks down on the kernel's H"
    model_replaced = tuple(k for k, (_, r) in enumerate(trace) if r)
    assert model_replaced == tuple(replaced), (model_replaced, replaced)
    g = gamma(n + 2)
    worst = {}
    if dt is LD:
        err, bound = np.abs(L @ L.T - Hk), g * (np.abs(L) @ np.abs(L).T)
    else:
        err, bound = np.abs(L @ L.T - Hk), 2.0 * g * (np.abs(L) @ np.abs(L).T)
        i, j = _sample(n, s.p1)
        Ll = L.astype(LD)
        es = np.abs((Ll[i] * Ll[j]).sum(axis=1) - _sym(out["normal"])[i, j])
        bs = g * (np.abs(Ll[i]) * np.abs(Ll[j])).sum(axis=1)
        on_replaced = np.isin(i, replaced) & (i == j)
        worst["factor (sampled in longdouble)"] = _worst(es[~on_replaced], bs[~on_replaced])
    exempt = np.zeros((n, n), dtype=bool)
    for k in replaced:
        exempt[k, k] = True
        assert out["factor"][k, k] == np.sqrt(out["normal"][k, k]), (k, out["factor"][k, k], np.sqrt(out["normal"][k, k]))
    worst["factor" if dt is LD else "factor (float64 BLAS, twice the bound)"] = _worst(err[low & ~exempt], bound[low & ~exempt])
    print("LPPIECES", shape_id(s), "replaced", model_replaced, "smallest pivot ratio",
          min(r for r, _ in trace), "error / bound:", {k: "%.3g" % v for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
    return worst


def check_solved(s, out, against_reference=True):
    """solved against the kernel's own L (the residual), and where no pivot was replaced and n < FULL_FROM against the
    longdouble solution of the reference H.  -> {name: largest error / bound}."""
    A, w, vm, vn = inputs(s)
    n = s.N + s.p1
    L = np.tril(out["factor"]).astype(LD)
    x = out["solved"].astype(LD)
    res = np.abs(L @ (L.T @ x) - vn.astype(LD))
    bound = gamma(3 * n + 2) * (np.abs(L) @ (np.abs(L).T @ np.abs(x)))
    worst = {"solved (residual)": _worst(res, bound)}
    if against_reference and n < FULL_FROM:
        xref, cond = _solution_reference(s.M, s.N, s.kind, s.p1)
        rel_err = float(np.linalg.norm((x - xref).astype(np.float64)) / np.linalg.norm(xref.astype(np.float64)))
        worst["solved (against the reference, cond %.3g)" % cond] = _worst(rel_err, cond * gamma(3 * n + s.M))
    print("LPPIECES", shape_id(s), "error / bound:", {k: "%.3g" % v for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
    return worst


def check_all(s, out, kernel, tag=""):
    """Every assertion of a 'random' shape (no pivot is replaced but the one of expected_replaced)."""
    check_poison_and_shape(s, out)
    worst = check_products(s, out, tag)
    replaced = expected_replaced(s)
    worst.update(check_factor(s, out, PIVOT[s.mode][kernel], replaced))
    worst.update(check_solved(s, out, against_reference=not replaced))
    return worst


def check_agreement(s, a, b, names=("normal", "factor", "u", "ax", "solved")):
    """Two kernels on one shape.  normal, u and ax within twice their bound of each other (each is within the bound of
    the exact value): an independent check, entry by entry.  The bounds of factor and solved are backward errors and do
    not carry over to the entries of L, so those two are compared where the bounds live, as L L^T and L L^T x, within
    the sum of the two kernels' bounds (plus twice normal's for L L^T).  That part follows from each kernel's own
    reference test and adds nothing new; it is kept so that every output appears in the comparison."""
    A, w, vm, vn = inputs(s)
    M, N, n = s.M, s.N, s.N + s.p1
    low = np.tri(n, dtype=bool)
    Af = bordered(A, s.p1, LD)
    S = np.abs(Af).T @ (np.abs(w).astype(LD)[:, None] * np.abs(Af))
    worst = {}
    worst["normal"] = _worst(np.abs(a["normal"] - b["normal"])[low], 2 * gamma(M + 3) * S[low])
    worst["u"] = _worst(np.abs(a["u"] - b["u"]), 2 * gamma(M + 3) * (np.abs(Af).T @ np.abs(vm).astype(LD)))
    worst["ax"] = _worst(np.abs(a["ax"] - b["ax"]), 2 * gamma(N + 3) * (np.abs(A).astype(LD) @ np.abs(vn[:N]).astype(LD)))
    assert a["ok"] == b["ok"] == 1
    La, Lb = np.tril(a["factor"]).astype(LD), np.tril(b["factor"]).astype(LD)
    Ga, Gb = La @ La.T, Lb @ Lb.T
    fb = gamma(n + 2) * (np.abs(La) @ np.abs(La).T + np.abs(Lb) @ np.abs(Lb).T) + 2 * gamma(M + 3) * S
    for k in expected_replaced(s):  # a replaced pivot's diagonal entry is exempt from the factor's bound
        low[k, k] = False
    worst["factor (as L L^T)"] = _worst(np.abs(Ga - Gb)[low], fb[low])
    xa, xb = a["solved"].astype(LD), b["solved"].astype(LD)
    ra, rb = La @ (La.T @ xa), Lb @ (Lb.T @ xb)
    sb = gamma(3 * n + 2) * (np.abs(La) @ (np.abs(La).T @ np.abs(xa)) + np.abs(Lb) @ (np.abs(Lb).T @ np.abs(xb)))
    worst["solved (as L L^T x)"] = _worst(np.abs(ra - rb), sb)
    print("LPPIECES agreement", shape_id(s), "error / bound:", {k: "%.3g" % v for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
    return worst
