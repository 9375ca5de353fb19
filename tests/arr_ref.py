"""The array combiner's specification in fp64 and integers with numpy (include/dpe_hip.h, "Antenna array combiner"),
and the two tolerance rules the GPU tests hold the device to.

With M elements, the block length L, block k = the samples [k L, (k + 1) L) cut to the record and x_a[n] = 0 outside it:
  S_k[a][b] = sum_n x_a[n] conj(x_b[n])         exact integers: Re = sum(I_a I_b + Q_a Q_b), Im = sum(Q_a I_b - I_a Q_b)
  R_k       = S_k + loading (tr S_k / M) I      fp64
  u         = R_k^-1 c_b,  w_b = u / (c_b^H u)
  fallback  w_b = c_b / (c_b^H c_b)  where block k holds fewer than 2 M samples of the record, tr S_k = 0, or u or w_b is not finite
  v_{b,a}   = fp32(gain conj(w_{b,a})) per component
  y_b[n]    = sum_a v_{b,a} x_a[n]

Tolerances, u = 2^-53 and 2^-24:
  weights  ||w^ - w||_2 <= 100 M^2 kappa_2(R) 2^-53 ||w||_2: Higham, Accuracy and Stability, Thm 10.4 (gamma_{3n+1}, n = 2 M for the
           real embedding of the Hermitian system), a factor n from the componentwise bound to norms, a factor 2 for LAPACK's own
           error in the reference
  output   per component, given the device's v: 2 M 1.01 2^-24 times the sum of the magnitudes of the component's 2 M terms, the
           bound of a 2 M-term FMA chain: sum_a(|v_re||x_I| + |v_im||x_Q|) for the real part, sum_a(|v_re||x_Q| + |v_im||x_I|) for the
           imaginary part."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def blocks_of(x, x_first, record_length, block_first, block_count, L):
    """x: complex [M, n] holding each element's samples from x_first on -> ([blocks, M, L] complex128 with zeros outside the record,
    samples inside the record per block [blocks]).  A sample of the record that the buffers do not hold is an error of the caller's."""
    x = np.asarray(x, dtype=np.complex128)
    M = x.shape[0]
    lo, hi = block_first * L, (block_first + block_count) * L
    b = hi if record_length is None else min(hi, record_length)
    flat = np.zeros((M, hi - lo), dtype=np.complex128)
    if b > lo:
        assert lo >= x_first and b <= x_first + x.shape[1], "the buffers do not hold the samples %d..%d" % (lo, b - 1)
        flat[:, :b - lo] = x[:, lo - x_first:b - x_first]
    count = np.clip(b - (lo + L * np.arange(block_count)), 0, L)
    return flat.reshape(M, block_count, L).transpose(1, 0, 2), count


def covariance(xb):
    """[blocks, M, L] complex with integer parts -> S int64 [blocks, M, M, 2], exactly"""
    I, Q = np.rint(xb.real).astype(np.int64), np.rint(xb.imag).astype(np.int64)
    re = np.einsum("kal,kbl->kab", I, I) + np.einsum("kal,kbl->kab", Q, Q)
    im = np.einsum("kal,kbl->kab", Q, I) - np.einsum("kal,kbl->kab", I, Q)
    return np.stack([re, im], axis=-1)


def loaded(S, loading):
    """R [blocks, M, M] complex128 of integer covariances S [blocks, M, M, 2]"""
    M = S.shape[1]
    tr = np.trace(S[..., 0], axis1=1, axis2=2)          # integers
    R = S[..., 0].astype(np.float64) + 1j * S[..., 1].astype(np.float64)
    return R + (loading * (tr.astype(np.float64) / M))[:, None, None] * np.eye(M), tr


def fallback_weights(cons):
    return cons / np.sum(np.abs(cons) ** 2, axis=-1, keepdims=True)


def weights(S, count, cons, loading):
    """-> (w complex128 [blocks, B, M], fallback bool [blocks, B], kappa_2(R) [blocks], nan where R is not used)"""
    cons = np.atleast_2d(np.asarray(cons, dtype=np.complex128))
    K, M, B = S.shape[0], S.shape[1], cons.shape[0]
    R, tr = loaded(S, loading)
    w = np.empty((K, B, M), dtype=np.complex128)
    fb = np.zeros((K, B), dtype=bool)
    kappa = np.full(K, np.nan)
    for k in range(K):
        if count[k] < 2 * M or tr[k] == 0:
            fb[k], w[k] = True, fallback_weights(cons)
            continue
        kappa[k] = np.linalg.cond(R[k])
        for b in range(B):
            with np.errstate(all="ignore"):
                try:
                    u = np.linalg.solve(R[k], cons[b])
                    wb = u / np.vdot(cons[b], u)
                except np.linalg.LinAlgError:
                    u = wb = np.full(M, np.nan)
            if not (np.all(np.isfinite(u.view(np.float64))) and np.all(np.isfinite(wb.view(np.float64)))):
                fb[k, b], wb = True, fallback_weights(cons[b])
            w[k, b] = wb
    return w, fb, kappa


def applied(w, gain):
    """v = fp32(gain conj(w)) per component, as float32 [..., 2]"""
    return np.stack([(gain * w.real).astype(np.float32), (-(gain * w.imag)).astype(np.float32)], axis=-1)


def unit_vector(M, reference):
    c = np.zeros((1, M), dtype=np.complex128)
    c[0, reference] = 1.0
    return c


def combine(x, x_first, record_length, out_first, out_count, L, v):
    """The apply in fp64 given v float32 [blocks, B, M, 2] for the blocks out_first div L .. (out_first + out_count - 1) div L ->
    (y complex128 [B, out_count], tol float64 [B, out_count, 2] per component)"""
    k0, k1 = out_first // L, (out_first + out_count - 1) // L
    xb, _ = blocks_of(x, x_first, record_length, k0, k1 - k0 + 1, L)
    M = xb.shape[1]
    vc = v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)          # [blocks, B, M]
    assert vc.shape[0] == k1 - k0 + 1
    y = np.einsum("kba,kal->bkl", vc, xb).reshape(vc.shape[1], -1)
    ar, ai, xi, xq = np.abs(vc.real), np.abs(vc.imag), np.abs(xb.real), np.abs(xb.imag)
    t_re = np.einsum("kba,kal->bkl", ar, xi) + np.einsum("kba,kal->bkl", ai, xq)
    t_im = np.einsum("kba,kal->bkl", ar, xq) + np.einsum("kba,kal->bkl", ai, xi)
    tol = 2 * M * 1.01 * U32 * np.stack([t_re.reshape(vc.shape[1], -1), t_im.reshape(vc.shape[1], -1)], axis=-1)
    a = out_first - k0 * L
    return y[:, a:a + out_count], tol[:, a:a + out_count]


def process(x, x_first, record_length, out_first, out_count, L, cons, loading=1e-3, gain=1.0):
    """The whole stage by the reference's own weights -> dict(y complex128 [B, out_count], S, w, v, fallback [blocks, B], kappa, count)
    over the blocks the outputs read"""
    k0, k1 = out_first // L, (out_first + out_count - 1) // L
    xb, count = blocks_of(x, x_first, record_length, k0, k1 - k0 + 1, L)
    S = covariance(xb)
    w, fb, kappa = weights(S, count, cons, loading)
    v = applied(w, gain)
    y, tol = combine(x, x_first, record_length, out_first, out_count, L, v)
    return dict(y=y, tol=tol, S=S, w=w, v=v, fallback=fb, kappa=kappa, count=count, k0=k0)


def counted(out_first, out_count, L, record_length=None):
    """the blocks a call counts: those whose first sample k L lies among its outputs and inside the record"""
    end = out_first + out_count if record_length is None else min(out_first + out_count, record_length)
    return [k for k in range(out_first // L, (out_first + out_count - 1) // L + 1) if out_first <= k * L < end]


def interleave(y):
    out = np.empty(2 * y.size, dtype=np.float64)
    out[0::2], out[1::2] = y.real, y.imag
    return out


def quantise(v):
    """clip(rint(.)) per component of an interleaved array, as int16"""
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def boundary_distance(v):
    """the distance of each value from the nearest rounding boundary (a half-integer)"""
    return np.abs(v - np.floor(v) - 0.5)
