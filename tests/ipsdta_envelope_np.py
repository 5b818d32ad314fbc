"""Host side of the IPSDTA envelope sweeps (tests/test_gpu_ipsdta_envelope.py, tests/test_gpu_tipsdta_envelope.py,
tests/test_ipsdta_envelope_cpu.py, tools/ipsdta_tolerance_probe.py --envelope): the grid, the seeded general states, the
restatements' outputs per entry point, the entry-wise metrics, the host conditions and the measured tolerances.  NumPy
only, but for `Device` at the end, the upload and call helper of the two GPU files, which imports torch when it is made.
The layout follows tests/envelope_np.py.

State.  `general_state(M, F, T, K, n_blocks, seed)`: X = ipsdta_np.mixture; W_f = a random complex unitary (QR of a complex
Gaussian) with its rows scaled by factors in [0.5, 1.5], well conditioned and not diagonally dominant; U per (source,
basis, block) = G G^H / nb + 0.1 I with G complex Gaussian, so every off-diagonal entry has a real and an imaginary part
and no two blocks are equal; H uniform in [0.1, 1.1]; ipsdta_np.normalize last.  `raw_state` is the same before that
normalisation: the normalised state has traces of one, where `normalize` is the identity up to a rounding and could not
tell a product from a quotient, so the `normalize` entry point alone is called on the raw U and H (its reference output
is then the general state itself).

Outputs (keys of `references`) and their entry-wise metrics, next to the family's pooled ones (tests/ipsdta_np.py):

    basis, normalize_U      per (source, basis, block) max|a - b| / max|b| over that block alone      pooled: basis_metric
    activation, normalize_H per entry |a - b| / |b|                                                   pooled: h_metric (same)
    spatial_1, spatial_2    per (bin, row) max|a - b| / max|b| (W after one sweep and after two)      pooled: w_metric
    loss                    ipsdta_np.loss_metric                                                     pooled: the same

Host conditions, asserted when a case is built (`case`), keep the comparison away from the switches where two correct
implementations may disagree: the activation numerator is never floored (min > 0); every clamped denominator (the
activation's, |eta| of the VCD step, the eigenvalues of R under the loss's logarithm, the singular values of W) and every
non-zero |eta_hat| is at least 1e6 eps; cond(R) < 1e3; every output is finite; and a host model of the kernels' LU
(`lu_row_swaps`: pivot on |re| + |im|, the first largest wins) swaps rows in at least one bin.

Tolerances.  Not read off a kernel.  `measure` gives, per output, the largest of (a) the LAPACK restatement against the
restatement on the kernels' own algorithms (la=KERNEL) and (b) the LAPACK restatement against itself after one_ulp /
herm_ulp of everything it reads, three draws.  `python tools/ipsdta_tolerance_probe.py --envelope` takes the largest over
the grid; D below is its output, rounded up to two digits, and `tolerance` makes 256 x d of it with a floor of 1e-13
(FACTOR and FLOOR64 of tests/envelope_np.py: two correct float64 implementations with different summation orders stay
within a few tens of d, a wrong entry is off by orders of magnitude).

The exception: `single_frame(case)`, T < M or T < the largest block.  Exactly one case may meet it (m5_f5_t1_k1_b1).  With
T < M, Q has rank T and is inverted through its eps shift alone, so no spatial reference exists for it (SPATIAL_CASES leaves
it out).  With T below the block size S_k has rank T and the square root of the basis update turns a rounding u into
sqrt(u), so its basis comparison gets 256 x ITS OWN d (D_BASIS_SINGLE_FRAME), pooled metric included (it cannot ask for
more than the entry-wise one).  Every other output of that case, and every other case, uses the common tolerance.

Output of the probe (d per case; `-` = no spatial reference), 2026-10:

    case                 model basis       activation  normalize_U normalize_H spatial_1   spatial_2   loss
    m8_f16_t65_k9_b2     gauss 1.1e-14     1.3e-15     5.9e-16     6.9e-16     7.7e-13     4.0e-13     2.7e-16
    m8_f16_t65_k9_b2     t     1.9e-14     1.1e-15     5.9e-16     6.9e-16     3.5e-13     5.1e-13     1.4e-16
    m7_f15_t63_k8_b3     gauss 1.2e-14     1.1e-15     5.9e-16     8.0e-16     3.1e-12     3.8e-12     1.2e-16
    m7_f15_t63_k8_b3     t     1.9e-14     1.0e-15     5.9e-16     8.0e-16     2.8e-12     2.5e-12     0.0e+00
    m6_f11_t64_k7_b2     gauss 1.3e-14     1.0e-15     4.8e-16     6.5e-16     3.7e-13     4.2e-13     1.9e-16
    m6_f11_t64_k7_b2     t     1.4e-14     1.0e-15     4.8e-16     6.5e-16     3.2e-13     3.7e-13     1.9e-16
    m8_f8_t130_k17_b1    gauss 2.8e-14     1.4e-15     6.0e-16     7.9e-16     6.7e-13     7.3e-13     1.8e-16
    m8_f8_t130_k17_b1    t     2.9e-14     1.3e-15     6.0e-16     7.9e-16     1.0e-12     1.1e-12     1.2e-16
    m4_f13_t257_k64_b2   gauss 4.1e-14     1.1e-15     6.4e-16     7.4e-16     2.3e-13     4.7e-13     2.0e-16
    m4_f13_t257_k64_b2   t     2.3e-14     1.1e-15     6.4e-16     7.4e-16     5.5e-13     5.1e-13     1.8e-16
    m5_f12_t40_k16_b3    gauss 1.0e-14     1.1e-15     6.4e-16     6.4e-16     2.3e-13     3.2e-13     1.7e-16
    m5_f12_t40_k16_b3    t     1.1e-14     1.1e-15     6.4e-16     6.4e-16     2.3e-13     3.1e-13     1.7e-16
    m3_f9_t577_k3_b4     gauss 4.2e-15     1.3e-15     4.8e-16     6.0e-16     2.4e-14     1.9e-14     1.1e-16
    m3_f9_t577_k3_b4     t     3.8e-15     9.3e-16     4.8e-16     6.0e-16     2.7e-14     3.5e-14     0.0e+00
    m2_f300_t8_k1_b300   gauss 1.1e-15     2.9e-16     4.4e-16     4.0e-16     2.0e-13     2.7e-13     0.0e+00
    m2_f300_t8_k1_b300   t     1.1e-15     4.8e-16     4.4e-16     4.0e-16     1.7e-13     1.6e-13     0.0e+00
    m3_f515_t9_k2_b257   gauss 5.3e-14     1.4e-15     6.8e-16     6.5e-16     9.1e-12     8.4e-12     3.1e-16
    m3_f515_t9_k2_b257   t     5.3e-14     1.5e-15     6.8e-16     6.5e-16     3.9e-12     4.6e-12     1.1e-16
    m5_f5_t1_k1_b1       gauss 1.9e-08     1.7e-15     4.0e-16     6.1e-16     -           -           1.1e-15
    m5_f5_t1_k1_b1       t     2.3e-08     7.2e-16     4.0e-16     6.1e-16     -           -           4.5e-16
"""
import functools

import numpy as np

import ipsdta_np as ip
import tipsdta_np as tp

EPS = 1e-12
FACTOR = 256.0
FLOOR64 = 1e-13
FAR = 1e6  # every clamped quantity of a grid case stays this many times above eps
COND_R_MAX = 1e3
N_DRAWS = 3
MODELS = ("gauss", "t")
NUS = (0.5, 4.0, 1000.0)

# name: (M, F, T, K, n_blocks, seed, nu of the Student-t model)
GRID = {
    "m8_f16_t65_k9_b2": (8, 16, 65, 9, 2, 101, 4.0),       # two blocks of 8 with M = 8: the largest footprint; K = KC + 1
    "m7_f15_t63_k8_b3": (7, 15, 63, 8, 3, 102, 0.5),       # M = 7, blocks of 5, no remainder group; K = KC
    "m6_f11_t64_k7_b2": (6, 11, 64, 7, 2, 103, 1000.0),    # M = 6, a block of 5 and one of 6: both groups; K = KC - 1
    "m8_f8_t130_k17_b1": (8, 8, 130, 17, 1, 104, 0.5),     # one block of 8; K = 17: two full chunks and one of one
    "m4_f13_t257_k64_b2": (4, 13, 257, 64, 2, 105, 4.0),   # blocks of 6 and 7; K = 64; T = 257
    "m5_f12_t40_k16_b3": (5, 12, 40, 16, 3, 106, 1000.0),  # M = 5, blocks of 4; K = 16: two exact chunks; T < 64
    "m3_f9_t577_k3_b4": (3, 9, 577, 3, 4, 107, 0.5),       # blocks of 2 and 3; three trips of the 256-thread frame loops
    "m2_f300_t8_k1_b300": (2, 300, 8, 1, 300, 108, 4.0),   # 300 blocks of one bin; F, n_blocks > 256; T below one wave
    "m3_f515_t9_k2_b257": (3, 515, 9, 2, 257, 109, 1000.0),  # 256 blocks of 2 and one of 3; F > 2 x 256
    "m5_f5_t1_k1_b1": (5, 5, 1, 1, 1, 110, 4.0),           # a single frame: T < M and T < block size (the exception)
}

KINDS = ("basis", "activation", "normalize_U", "normalize_H", "spatial", "loss")

# ---------------------------------------------------------------------------------------------------------- measured
# Output of `python tools/ipsdta_tolerance_probe.py --envelope`: the largest d over the grid per model and output, rounded
# up to two digits.
D = {
    "gauss": {"basis": 5.4e-14, "activation": 1.7e-15, "normalize_U": 6.8e-16, "normalize_H": 8.1e-16, "spatial": 9.1e-12,
              "loss": 1.1e-15},
    "t": {"basis": 5.3e-14, "activation": 1.5e-15, "normalize_U": 6.8e-16, "normalize_H": 8.1e-16, "spatial": 4.6e-12,
          "loss": 4.5e-16},
}
# update_basis of the single-frame case: its own d (see the module docstring)
D_BASIS_SINGLE_FRAME = {
    "gauss": {"m5_f5_t1_k1_b1": 2.0e-8},
    "t": {"m5_f5_t1_k1_b1": 2.3e-8},
}


def tolerance(d, floor=FLOOR64):
    return max(FACTOR * d, floor)


def kind_of(output):
    """spatial_1, spatial_2 -> spatial; every other output is its own kind"""
    return "spatial" if output.startswith("spatial") else output


def block_sizes(case):
    M, F, T, K, nblk = GRID[case][:5]
    return [nb for _, _, nb in ip.part_ranges(F, nblk)]


def single_frame(case):
    """T < M (Q has rank T) or T < the largest block (S_k has rank T)"""
    M, F, T = GRID[case][:3]
    return T < M or T < max(block_sizes(case))


SPATIAL_CASES = tuple(c for c in GRID if GRID[c][2] >= GRID[c][0])


def entry_tolerance(case, model, output):
    """The entry-wise tolerance of one output (keys of `references`) of one grid case."""
    kind = kind_of(output)
    if kind == "basis" and single_frame(case):
        return tolerance(D_BASIS_SINGLE_FRAME[model][case])
    return tolerance(D[model][kind])


def pooled_tolerance(case, model, output):
    """The family's own bound on the pooled metric: the one-stage figure of tolerances.json (normalize: the bound of
    tests/test_gpu_ipsdta.py, (F + 1) 2^-52); never below the entry-wise tolerance where that is the exception's."""
    kind = kind_of(output)
    if kind.startswith("normalize"):
        return (GRID[case][1] + 1) * 2.0 ** -52
    tol = (ip if model == "gauss" else tp).tolerances()["one_stage"]
    t = tol[{"basis": "U", "activation": "H", "spatial": "W", "loss": "loss"}[kind]]
    return max(t, entry_tolerance(case, model, output)) if kind == "basis" and single_frame(case) else t


# ---------------------------------------------------------------------------------------------------------- metrics
def block_metric(a, b):
    """per (source, basis, block) max|a - b| / max|b| over that block alone, the largest"""
    worst = 0.0
    for pa, pb in zip(ip.to_parts(a), ip.to_parts(b)):
        worst = max(worst, float(np.max(np.max(np.abs(pa - pb), axis=(-2, -1)) / np.max(np.abs(pb), axis=(-2, -1)))))
    return worst


def row_metric(a, b):
    """per (bin, row) max|a - b| / max|b|, the largest"""
    return float(np.max(np.max(np.abs(a - b), axis=-1) / np.max(np.abs(b), axis=-1)))


def _finite(a):
    return all(np.all(np.isfinite(p)) for p in (a if isinstance(a, (tuple, list)) else (a,)))


def entrywise(case, output, a, b):
    assert _finite(a), "non-finite output"
    kind = kind_of(output)
    if kind in ("basis", "normalize_U"):
        return block_metric(a, b)
    if kind in ("activation", "normalize_H"):
        return ip.h_metric(a, b)
    if kind == "spatial":
        return row_metric(a, b)
    M, F, T = GRID[case][:3]
    return ip.loss_metric(a, b, M, F, T)


def pooled(case, output, a, b):
    kind = kind_of(output)
    if kind in ("basis", "normalize_U"):
        return ip.basis_metric(a, b)
    if kind in ("activation", "normalize_H"):
        return ip.h_metric(a, b)
    if kind == "spatial":
        return ip.w_metric(a, b)
    M, F, T = GRID[case][:3]
    return ip.loss_metric(a, b, M, F, T)


# ---------------------------------------------------------------------------------------------------------- states
def raw_state(M, F, T, K, n_blocks, seed):
    """(X, W, basis, H) before the normalisation"""
    X = ip.mixture(M, F, T, seed)
    rng = np.random.default_rng((seed, 1))
    q = np.linalg.qr(rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M)))[0]
    W = np.ascontiguousarray((0.5 + rng.random((F, M, 1))) * q)
    parts = []
    for _, n, nb in ip.part_ranges(F, n_blocks):
        G = rng.standard_normal((M, K, n, nb, nb)) + 1j * rng.standard_normal((M, K, n, nb, nb))
        A = G @ ip.ct(G) / nb + 0.1 * np.eye(nb)
        parts.append((A + ip.ct(A)) / 2)
    H = 0.1 + rng.random((M, K, T))
    return X, W, ip.from_parts(parts, F, n_blocks), H


def general_state(M, F, T, K, n_blocks, seed):
    X, W, U, H = raw_state(M, F, T, K, n_blocks, seed)
    U, H = ip.normalize(U, H, F, n_blocks)
    return X, W, U, H


def state(case):
    return general_state(*GRID[case][:6])


def nu_of(case, model):
    return None if model == "gauss" else GRID[case][6]


# ---------------------------------------------------------------------------------------------------------- references
def references(case, model, st=None, raw=None, la=ip.LAPACK, diag=None):
    """Every entry point of the restatement on ONE state (not chained): basis, activation, normalize_U, normalize_H (of
    the raw state), spatial_1 and spatial_2 (where the case has a spatial reference), loss."""
    M, F, T, K, nblk, seed, nu = GRID[case]
    X, W, U, H = state(case) if st is None else st
    raw = raw_state(M, F, T, K, nblk, seed) if raw is None else raw
    rs, ex = (ip, ()) if model == "gauss" else (tp, (nu,))
    out = {"basis": rs.update_basis(X, W, U, H, EPS, nblk, *ex, la),
           "activation": rs.update_activation(X, W, U, H, EPS, nblk, *ex, la, diag=diag)}
    out["normalize_U"], out["normalize_H"] = ip.normalize(raw[2], raw[3], F, nblk)
    if case in SPATIAL_CASES:
        out["spatial_1"], out["spatial_2"] = rs.update_spatial(X, W, U, H, EPS, nblk, *ex, 2, la, each=True, diag=diag)
    out["loss"] = np.float64(rs.loss(X, W, U, H, EPS, nblk, *ex, la))
    return out


def lu_row_swaps(W):
    """The number of bins in which the kernels' LU of W_f (partial pivoting on |re| + |im|, a later row wins only where
    it is strictly larger) swaps rows at least once."""
    bins = 0
    for A in np.array(W, dtype=np.complex128):
        M = A.shape[0]
        swapped = False
        for j in range(M):
            s = np.abs(A[j:, j].real) + np.abs(A[j:, j].imag)
            p = j + int(np.argmax(s))  # argmax returns the first of equal entries
            if p != j:
                A[[j, p]] = A[[p, j]]
                swapped = True
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j] / A[j, j], A[j, j + 1:])
        bins += swapped
    return bins


def host_conditions(case, st, refs, diags):
    """Assert the conditions of the module docstring; returns the figures."""
    X, W, U, H = st
    fig = {"cond_R": ip.max_cond(U, H, EPS), "swaps": lu_row_swaps(W),
           "sv_W": float(np.min(np.linalg.svd(W, compute_uv=False)))}
    fig["eig_R"] = min(float(np.min(np.linalg.eigvalsh(ip.to_psd(np.einsum("nkt,nkbij->ntbij", H, Up), EPS))))
                       for Up in ip.to_parts(U))
    assert fig["cond_R"] < COND_R_MAX, (case, fig)
    assert fig["eig_R"] >= FAR * EPS and fig["sv_W"] >= FAR * EPS, (case, fig)
    assert fig["swaps"] >= 1, (case, "the LU never swaps rows")
    for model in MODELS:
        d = diags[model]
        fig[model] = d
        assert d["num_min"] > 0.0 and not d["num_floored"], (case, model, d)
        assert d["den_min"] >= FAR * EPS, (case, model, d)
        if case in SPATIAL_CASES:
            assert d["eta_min"] >= FAR * EPS, (case, model, d)
            assert d.get("eta_hat_min", np.inf) >= FAR * EPS, (case, model, d)
        assert all(_finite(v) for v in refs[model].values()), (case, model)
    return fig


@functools.lru_cache(maxsize=None)
def case(name):
    """(state, raw U, raw H, {model: references}) of a grid case, computed once, with the host conditions asserted.  The
    arrays are shared among the tests: nobody writes to them."""
    M, F, T, K, nblk, seed, nu = GRID[name]
    raw = raw_state(M, F, T, K, nblk, seed)
    st = state(name)
    refs, diags = {}, {}
    for model in MODELS:
        diags[model] = {}
        refs[model] = references(name, model, st, raw, diag=diags[model])
    host_conditions(name, st, refs, diags)
    for a in st + raw[2:]:
        for p in (a if isinstance(a, tuple) else (a,)):
            p.setflags(write=False)
    return st, raw[2], raw[3], refs


# ---------------------------------------------------------------------------------------------------------- probe
def perturbed(st, rng):
    X, W, U, H = st
    return ip.one_ulp(X, rng), ip.one_ulp(W, rng), ip.herm_ulp(U, rng), ip.one_ulp(H, rng)


def measure(name, model, draws=N_DRAWS):
    """{output: d}: the largest entry-wise difference between the LAPACK restatement and (a) the restatement on the
    kernels' algorithms, (b) itself after a one-ulp move of everything it reads (`draws` draws of the directions)."""
    M, F, T, K, nblk, seed, nu = GRID[name]
    st, raw = state(name), raw_state(M, F, T, K, nblk, seed)
    base = references(name, model, st, raw)
    others = [references(name, model, st, raw, la=ip.KERNEL)]
    for k in range(draws):
        rng = np.random.default_rng((seed, 2, k))
        others.append(references(name, model, perturbed(st, rng), perturbed(raw, rng)))
    return {out: max(entrywise(name, out, o[out], base[out]) for o in others) for out in base}


def measure_grid(names=None, models=MODELS, draws=N_DRAWS, report=None):
    """({model: {kind: d}}, {model: {case: d}} of the single-frame basis) over `names` (default: the grid)"""
    worst = {m: {k: 0.0 for k in KINDS} for m in models}
    own = {m: {} for m in models}
    for name in (names or GRID):
        for m in models:
            d = measure(name, m, draws)
            if report:
                report(name, m, d)
            for out, v in d.items():
                k = kind_of(out)
                if k == "basis" and single_frame(name):
                    own[m][name] = v
                else:
                    worst[m][k] = max(worst[m][k], v)
    return worst, own


def round_up(d, digits=2):
    """d rounded up to `digits` significant digits"""
    if d == 0.0:
        return 0.0
    e = int(np.floor(np.log10(d))) - (digits - 1)
    return float("%.*e" % (digits - 1, np.ceil(d / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e))


# ---------------------------------------------------------------------------------------------------------- device side
# For the two GPU files only; torch and the package are imported when a Device is made, not with this module.
class Device:
    """One grid case on the device, as the entry points of `model` take it: X (M,F,T), W (F,M,M), the packed basis
    (N,K,P), H (N,K,T), workspace and status.  raw=True uploads the basis and activation before their normalisation."""

    def __init__(self, eng, name, model, raw=False):
        from audio_source_separation_amd._device import to_device, torch
        M, F, T, K, nblk, _, nu = GRID[name]
        (X, W, U, H), rawU, rawH, _ = case(name)
        if raw:
            U, H = rawU, rawH
        self.eng, self.name, self.model, self.F, self.nblk = eng, name, model, F, nblk
        self.host = {"X": np.ascontiguousarray(X), "W": np.ascontiguousarray(W), "U": ip.pack(U), "H": np.ascontiguousarray(H)}
        self.X = to_device(self.host["X"], torch.complex128, eng.dev)
        self.W = to_device(self.host["W"], torch.complex128, eng.dev)
        self.U = to_device(self.host["U"], torch.complex128, eng.dev)
        self.H = to_device(self.host["H"], torch.float64, eng.dev)
        self.tail = () if model == "gauss" else (nu,)
        self.ws = eng.ipsdta_workspace(M, F, T, K, nblk) if model == "gauss" else eng.tipsdta_workspace(M, F, T, K, nblk, nu)
        self.status = eng.new_status(1)

    def call(self, entry, **kwargs):
        """Engine.ipsdta_<entry> or Engine.tipsdta_<entry> on the uploaded state; returns what the entry point returns"""
        fn = getattr(self.eng, ("ipsdta_" if self.model == "gauss" else "tipsdta_") + entry)
        return fn(self.X, self.W, self.U, self.H, self.ws, self.nblk, *self.tail, eps=EPS, status=self.status, **kwargs)

    def fetch(self):
        """{"X", "W", "U" (packed), "H"} as they stand on the device, after asserting status 0"""
        from audio_source_separation_amd._device import to_numpy
        got = {k: to_numpy(getattr(self, k)) for k in ("X", "W", "U", "H")}
        assert int(self.status.item()) == 0, (self.name, "status", int(self.status.item()))
        return got

    def basis(self, got):
        return ip.unpack(got["U"], self.F, self.nblk)

    def unchanged(self, got, owned):
        """the arrays the call does not own are bit for bit what was uploaded"""
        for k in ("X", "W", "U", "H"):
            if k not in owned:
                assert np.array_equal(got[k], self.host[k]), (self.name, k, "changed")


def check(name, model, output, got):
    """Print, then assert, the pooled and the entry-wise figure of one output against the cached reference."""
    want = case(name)[3][model][output]
    p, ptol = pooled(name, output, got, want), pooled_tolerance(name, model, output)
    e, etol = entrywise(name, output, got, want), entry_tolerance(name, model, output)
    print("%s %s %s: pooled %.3e (<= %.2e)  entry-wise %.3e (<= %.2e)" % (name, model, output, p, ptol, e, etol))
    assert p <= ptol, (name, model, output, "pooled", p, ptol)
    assert e <= etol, (name, model, output, "entry-wise", e, etol)
