"""NumPy restatement of GaussIDLMA (src/sss/idlma.py:89-246 of the reference), the two test networks, and NumPy models of
what the kernels of csrc/assx_idlma.hip do differently.  Shared by tests/golden/idlma/make_idlma.py,
tools/idlma_tolerance_probe.py and the tests; no GPU, no reference import.

Arrays: X (M,F,T) complex128, W (F,N,M) complex128, the network's input, raw output and dnn_output d (N,F,T) float32.

The float32 points (each a `fault=` that restates it wrongly, for the tests that the fixtures notice):
  network input   float32(P**(domain/2)), P = |W x|^2 in float64
  d               raw**(2/domain) on a float32 array: float32 arithmetic           fault "f64_square": d widened, float64 on
                  floored at float32(dnn_flooring) AFTER that exponent             fault "floor_first": floored before it
  R               d**(2/domain) AGAIN, float32, floored at float32(eps)            fault "single_exponent": R = d
  loss            after normalisation                                              fault "loss_before_normalize"
"""
import numpy as np
import torch

try:
    from audio_source_separation_amd._lib import IDLMA_FRAME_CHUNK as FRAME_CHUNK
except Exception:  # the library is not built where the fixtures are made
    FRAME_CHUNK = 1024

N_ITER = 10
THRESHOLD = 1e12
VEC = 4  # frames of one thread of the pass over X

# envelope frames: beamform_envelope_np.FRAMES plus T = M (added per problem) and the kernels' own seams: a partial and a
# whole vector store (T % 4), one frame past a chunk
ENVELOPE_EXTRA_FRAMES = (66, 68, FRAME_CHUNK + 4)

CASES = (
    # name, M, F, T, domain, net, seed, options
    ("idlma_m2_f5_t32_d2", 2, 5, 32, 2, "exact", 11, {}),
    ("idlma_m3_f7_t48_d1", 3, 7, 48, 1, "exact", 12, {}),
    ("idlma_m2_f5_t32_d15", 2, 5, 32, 1.5, "exact", 13, {}),
    ("idlma_m4_f9_t64_d2_matmul", 4, 9, 64, 2, "matmul", 14, {}),
    ("idlma_m8_f6_t40_d2", 8, 6, 40, 2, "exact", 15, {}),
    ("idlma_m2_f17_t96_d2_epsfloor", 2, 17, 96, 2, "exact", 16, {"dnn_flooring": 0.0, "zero_g": True}),
    ("idlma_m3_f7_t48_d1_dnnfloor", 3, 7, 48, 1, "exact", 27, {"zero_g": True}),  # seed 17: cond 7.0e6
    ("idlma_m3_f5_t40_d2_ref1", 3, 5, 40, 2, "exact", 18, {"reference_id": 1}),
)


# ------------------------------------------------------------------------------------------------------ inputs, networks
def convolutive_mixture(M, F, T, seed, n_basis=3):
    """Low-rank-variance complex Gaussian sources mixed by a random matrix per bin."""
    rng = np.random.default_rng(seed)
    S = np.empty((M, F, T), dtype=np.complex128)
    for n in range(M):
        var = (rng.random((F, n_basis)) ** 2) @ (rng.random((n_basis, T)) ** 4) + 1e-3
        S[n] = np.sqrt(var / 2) * (rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T)))
    A = rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))
    return np.einsum("fmn,nft->mft", A, S)


class ExactNet(torch.nn.Module):
    """(0.5 x + 0.25 roll(x, 1, -1) + 0.25 roll(x, -1, -1)) g: element-wise, correctly rounded operations only, so a CPU
    and a GPU give the same bits."""

    def __init__(self, g):
        super().__init__()
        self.g = torch.nn.Parameter(torch.as_tensor(np.asarray(g, dtype=np.float32)), requires_grad=False)

    def forward(self, x):
        return (0.5 * x + 0.25 * torch.roll(x, 1, -1) + 0.25 * torch.roll(x, -1, -1)) * self.g


class MatmulNet(torch.nn.Module):
    """A mask on x from Linear F -> 16, ReLU, Linear 16 -> F, sigmoid along the bins; no convolution, nothing recurrent."""

    def __init__(self, w1, b1, w2, b2):
        super().__init__()
        f32 = lambda a: torch.nn.Parameter(torch.as_tensor(np.asarray(a, dtype=np.float32)), requires_grad=False)  # noqa: E731
        self.w1, self.b1, self.w2, self.b2 = f32(w1), f32(b1), f32(w2), f32(b2)

    def forward(self, x):
        h = torch.relu(x.transpose(1, 2) @ self.w1.T + self.b1)
        return x * torch.sigmoid(h @ self.w2.T + self.b2).transpose(1, 2)


def draw_net(kind, M, F, T, seed, zero_g=False):
    """The stored arrays of a network (a dict of float32 arrays whose keys start with net_)."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "exact":
        g = (0.5 + rng.random((M, F, 1 if seed % 2 else T))).astype(np.float32)
        if zero_g:  # M + 2 frames of one (source, bin) silent: fewer than T - M, the bin stays well conditioned
            g = np.ascontiguousarray(np.broadcast_to(g, (M, F, T))).copy()
            g[0, min(3, F - 1), :M + 2] = 0.0
        return {"net_g": g}
    return {"net_w1": (rng.standard_normal((16, F)) / np.sqrt(F)).astype(np.float32),
            "net_b1": (0.1 * rng.standard_normal(16)).astype(np.float32),
            "net_w2": (rng.standard_normal((F, 16)) / 4).astype(np.float32),
            "net_b2": (0.1 * rng.standard_normal(F)).astype(np.float32)}


def build_net(fx, device="cpu"):
    """The network of a fixture (or of draw_net's dict) on `device`."""
    if "net_g" in fx:
        net = ExactNet(fx["net_g"])
    else:
        net = MatmulNet(fx["net_w1"], fx["net_b1"], fx["net_w2"], fx["net_b2"])
    return net.to(device)


def run_net(net, x):
    with torch.no_grad():
        return net(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def params(fx):
    return dict(domain=float(fx["domain"]), dnn_flooring=float(fx["dnn_flooring"]), eps=float(fx["eps"]),
                reference_id=int(fx["reference_id"]))


# ------------------------------------------------------------------------------------------------------ the restatement
def separate(X, W):
    return (W @ X.transpose(1, 0, 2)).transpose(1, 0, 2)


def power(X, W):
    return np.abs(separate(X, W)) ** 2


def network_input(X, W, domain):
    return (power(X, W) ** (domain / 2)).astype(np.float32)


def source_output(raw, domain, dnn_flooring, fault=None):
    raw = np.asarray(raw, dtype=np.float32)
    if fault == "floor_first" and dnn_flooring:
        raw = np.maximum(raw, dnn_flooring)
    d = raw.astype(np.float64) ** (2 / domain) if fault == "f64_square" else raw ** (2 / domain)
    if dnn_flooring and fault != "floor_first":
        d = np.maximum(d, dnn_flooring)
    return d


def variance(d, domain, eps, fault=None):
    R = np.array(d, copy=True) if fault == "single_exponent" else d ** (2 / domain)
    R[R < eps] = eps
    return R


def space_update(X, W, R, threshold=THRESHOLD):
    """One IP sweep (idlma.py:195-208) with U_n = mean_t x x^H / R_n; R (N,F,T)."""
    M, F, T = X.shape
    W = W.copy()
    Xf = X.transpose(1, 2, 0)  # (F,T,M)
    XX = Xf[..., :, None] * Xf[..., None, :].conj()  # (F,T,M,M)
    E = np.eye(M)
    for n in range(M):
        Un = (XX / R[n][..., None, None]).mean(axis=1)  # (F,M,M)
        WU = W @ Un
        ok = np.linalg.cond(WU) < threshold
        w = np.linalg.solve(WU, np.broadcast_to(E[n][:, None], (F, M, 1)))[..., 0]
        den = np.sqrt(np.einsum("fi,fij,fj->f", w.conj(), Un, w))
        W[:, n, :] = np.where(ok[:, None], w.conj() / den[:, None], W[:, n, :])
    return W


def pb_scale(Y, ref):
    """scale (N,F) = (x_ref Y^H (Y Y^H)^-1)[n] per bin (projection_back.py:13-21); ref (F,T)."""
    Yf = Y.transpose(1, 0, 2)
    YH = Yf.transpose(0, 2, 1).conj()
    A = ref[:, None, :] @ YH @ np.linalg.inv(Yf @ YH)
    return A[:, 0, :].T


def normalize_refit(X, Y, scale):
    """idlma.py:152-155: W = (Y scale) X^H (X X^H)^-1."""
    Xf = X.transpose(1, 0, 2)
    XH = Xf.transpose(0, 2, 1).conj()
    return (Y * scale[..., None]).transpose(1, 0, 2) @ XH @ np.linalg.inv(Xf @ XH)


def normalize_scaled(W, scale):
    """what the kernel does: W[f,n,:] *= scale[n,f]."""
    return W * scale.T[:, :, None]


def loss(X, W, d, domain, eps, fault=None, R=None):
    """R: the float32 variance where it is not to be formed from d"""
    T = X.shape[2]
    P = power(X, W)
    R = variance(d, domain, eps, fault) if R is None else R
    return np.sum(P / R + np.log(R)) - 2 * T * np.sum(np.log(np.abs(np.linalg.det(W))))


def iterate(X, W, net, domain, dnn_flooring, eps, reference_id, fault=None, form="refit", raw=None, trace=None):
    """One update_once and the loss after it: (W, d, loss).  raw: the network's output where it is not to be evaluated."""
    inp = network_input(X, W, domain)
    if raw is None:
        raw = run_net(net, inp)
    d = source_output(raw, domain, dnn_flooring, fault)
    W_ip = space_update(X, W, variance(d, domain, eps, fault))
    Y = separate(X, W_ip)
    scale = pb_scale(Y, X[reference_id])
    W_new = normalize_refit(X, Y, scale) if form == "refit" else normalize_scaled(W_ip, scale)
    value = loss(X, W_ip if fault == "loss_before_normalize" else W_new, d, domain, eps, fault)
    if trace is not None:
        trace.append(dict(inp=inp, raw=raw, d=d, W_ip=W_ip, scale=scale, W=W_new))
    return W_new, d, value


def output(X, W, reference_id):
    Y = separate(X, W)
    return Y * pb_scale(Y, X[reference_id])[..., None]


def run(X, net, domain, dnn_flooring, eps, reference_id, n_iter=N_ITER, fault=None, form="refit", trace=None):
    """The front door from the identity: (W, d, losses, output)."""
    M, F, T = X.shape
    W = np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1))
    d = np.ones((M, F, T))
    losses = [loss(X, W, d, domain, eps)]
    for _ in range(n_iter):
        W, d, value = iterate(X, W, net, domain, dnn_flooring, eps, reference_id, fault, form, trace=trace)
        losses.append(value)
    return W, d, np.array(losses), output(X, W, reference_id)


# ------------------------------------------------------------------------------------------------------ kernel models
def kernel_loss(X, W, d, domain, eps, R=None):
    """The loss as assx_idlma_loss adds it up: log R the float64 logarithm rounded to float32; a thread's four frames and
    the sources in index order, a wave's butterfly, the waves of a workgroup, the workgroups, then the bins' ln|det|."""
    M, F, T = X.shape
    R32 = variance(np.asarray(d, dtype=np.float32), domain, eps) if R is None else np.asarray(R, dtype=np.float32)
    R = R32.astype(np.float64)
    term = power(X, W) / R + np.log(R).astype(np.float32).astype(np.float64)  # (N,F,T)
    CH = -(-T // FRAME_CHUNK)
    pad = np.zeros((M, F, CH * FRAME_CHUNK))
    pad[:, :, :T] = term
    th = np.zeros((F, CH, FRAME_CHUNK // VEC))
    for k in range(VEC):
        for n in range(M):
            th += pad[n].reshape(F, CH, FRAME_CHUNK // VEC, VEC)[..., k]
    wv = th.reshape(F, CH, -1, 64)
    for off in (32, 16, 8, 4, 2, 1):
        wv = wv[..., :off] + wv[..., off:2 * off]
    part = np.zeros((F, CH))
    for w in range(wv.shape[2]):
        part += wv[:, :, w, 0]
    ld = np.log(np.abs(np.linalg.det(W)))
    return strided_sum(part.reshape(-1)) - 2.0 * T * strided_sum(ld)


def strided_sum(v, blk=256):
    """every thread its own stride of blk, a wave's butterfly, the waves in index order"""
    th = np.zeros(blk)
    for i in range(0, len(v), blk):
        seg = v[i:i + blk]
        th[:len(seg)] += seg
    wv = th.reshape(-1, 64)
    for off in (32, 16, 8, 4, 2, 1):
        wv = wv[:, :off] + wv[:, off:2 * off]
    tot = 0.0
    for w in range(wv.shape[0]):
        tot += wv[w, 0]
    return tot


# ------------------------------------------------------------------------------------------------------ metrics, moves
def w_metric(a, b):
    """per bin max|a - b| / max|b|, the largest bin"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b).reshape(len(b), -1).max(axis=1) / np.abs(b).reshape(len(b), -1).max(axis=1)))


def d_metric(a, b):
    """entry-wise |a - b| / |b| of a positive map; an entry on the floor (equal in both) counts 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))


def loss_metric(a, b, X):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + X.size)))


def out_metric(a, b):
    """per source max|a - b| / max|b|"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b).reshape(len(b), -1).max(axis=1) / np.abs(b).reshape(len(b), -1).max(axis=1)))


def one_ulp(a, rng):
    """every real and imaginary part moved to a neighbouring number of its type, the direction drawn"""
    a = np.array(a, copy=True)
    v = a.view(np.float64 if a.dtype in (np.complex128, np.float64) else np.float32)
    step = rng.integers(0, 2, v.shape) * 2 - 1
    v[...] = np.nextafter(v, np.where(step > 0, np.inf, -np.inf).astype(v.dtype))
    return a
