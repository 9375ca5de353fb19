"""The excisor's specification in fp64 with numpy (include/dpe_hip.h, "Interference excision"), the two tolerance
rules the GPU tests hold the device to, and the decided-bin rule.

With the frame length N, the hop H = N / 2 and x[n] = 0 outside [0, record_length):
  b[n]   = 0 where |x[n]|^2 > blank_power (blank_power = 0: off), else x[n]
  X_k[f] = sum_i w[i] b[(k - 1) H + i] exp(-2 pi j f i / N),   w[i] = sin(pi (i + 1/2) / N)
  P_k    = |X_k|^2,  m_k = sort(P_k)[N / 2 - 1],  detected where P_k > kappa m_k (strict)
  e_k[f] = static[f] or a detected bin within +-guard of f, cyclically
  y_k    = ifft(X_k (1 - e_k)),   out[n] = gain (w[r + H] y_h[r + H] + w[r] y_{h+1}[r]),  h = n div H, r = n mod H

Tolerances, u = 2^-24, c = 12 (Higham, Accuracy and Stability, Thm 24.2 gives 6.7 log2 N u for the fp32 transform's 2-norm error):
  per bin   |X^ - X| <= E_k = c log2 N u sqrt(N) ||fr_k||_2, so |P^ - P| <= delta = 2 |X| E_k + E_k^2 + 4 u P
  output    tol[n] = |gain| (t_h + t_{h+1} + 8 u (|y_h[r + H]| + |y_{h+1}[r]|)),  t_k = 2 c log2 N u ||fr_k||_2
with fr_k the windowed, blanked frame."""
import numpy as np

U = 2.0 ** -24
C_FFT = 12.0


def window(N):
    return np.sin(np.pi * (np.arange(N) + 0.5) / N)


def from_i16(iq):
    """interleaved int16 -> complex128"""
    v = np.asarray(iq).astype(np.float64)
    return v[0::2] + 1j * v[1::2]


def interleave(y):
    out = np.empty(2 * y.size, dtype=np.float64)
    out[0::2], out[1::2] = y.real, y.imag
    return out


def quantise(v):
    """clip(rint(.)) per component of an interleaved array, as int16"""
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def blanked(x, blank_power):
    """the samples the blanker zeroes"""
    if blank_power <= 0:
        return np.zeros(x.shape, dtype=bool)
    return x.real ** 2 + x.imag ** 2 > blank_power


def samples(x, x_first, record_length, lo, hi, blank_power=0.0):
    """b[lo .. hi): `x` holds the record's samples from x_first on; what the record does not hold is zero.  A sample of the record
    that the buffer does not hold is an error of the caller's."""
    x = np.asarray(x, dtype=np.complex128)
    a, b = max(lo, 0), hi if record_length is None else min(hi, record_length)
    out = np.zeros(hi - lo, dtype=np.complex128)
    if b > a:
        assert a >= x_first and b <= x_first + x.size, "the buffer does not hold the samples %d..%d" % (a, b - 1)
        seg = x[a - x_first:b - x_first].copy()
        seg[blanked(seg, blank_power)] = 0.0
        out[a - lo:b - lo] = seg
    return out


def windowed(x, x_first, record_length, frame_first, frame_count, N, blank_power=0.0):
    """fr_k for the frames [frame_first, frame_first + frame_count): [frames, N]"""
    H = N // 2
    b = samples(x, x_first, record_length, (frame_first - 1) * H, (frame_first + frame_count) * H, blank_power)
    idx = np.arange(frame_count)[:, None] * H + np.arange(N)[None, :]
    return b[idx] * window(N)[None, :]


def lower_median(P):
    return np.sort(P, axis=-1)[..., P.shape[-1] // 2 - 1]


def widen(detected, guard, static=None):
    """e = static or a detected bin within +-guard, cyclically (last axis)"""
    e = np.zeros(detected.shape, dtype=bool)
    for d in range(-guard, guard + 1):
        e |= np.roll(detected, d, axis=-1)
    if static is not None:
        e |= np.asarray(static, dtype=bool)
    return e


def frames(x, x_first, record_length, frame_first, frame_count, N, kappa, guard, static=None, blank_power=0.0):
    """-> dict(fr, X, P, m, detected, e) of the frames [frame_first, frame_first + frame_count), each [frames, N] (m: [frames])"""
    fr = windowed(x, x_first, record_length, frame_first, frame_count, N, blank_power)
    X = np.fft.fft(fr, axis=-1)
    P = X.real ** 2 + X.imag ** 2
    m = lower_median(P)
    detected = P > kappa * m[:, None]
    return dict(fr=fr, X=X, P=P, m=m, detected=detected, e=widen(detected, guard, static))


def excise(x, x_first, record_length, out_first, out_count, N, kappa, guard, static=None, blank_power=0.0, gain=1.0, masks=None, detail=False):
    """out[out_first .. out_first + out_count) as complex128.  masks: e for the frames out_first div H .. (out_first + out_count - 1)
    div H + 1 in place of the reference's own detection ([frames, N]).  detail: -> (out, tol, frames dict)."""
    H = N // 2
    k0, k1 = out_first // H, (out_first + out_count - 1) // H + 1
    F = frames(x, x_first, record_length, k0, k1 - k0 + 1, N, kappa, guard, static, blank_power)
    e = F["e"] if masks is None else np.asarray(masks, dtype=bool)
    assert e.shape == F["X"].shape
    y = np.fft.ifft(F["X"] * ~e, axis=-1)
    w = window(N)
    n = out_first + np.arange(out_count)
    h, r = n // H - k0, n % H
    first, second = w[r + H] * y[h, r + H], w[r] * y[h + 1, r]
    out = gain * (first + second)
    if not detail:
        return out
    t = 2.0 * C_FFT * np.log2(N) * U * np.linalg.norm(F["fr"], axis=-1)
    tol = abs(gain) * (t[h] + t[h + 1] + 8.0 * U * (np.abs(y[h, r + H]) + np.abs(y[h + 1, r])))
    F["e_used"] = e
    return out, tol, F


def power_tolerance(F, N):
    """delta [frames, N]: the bound on |P^ - P| of a frames() result"""
    E = C_FFT * np.log2(N) * U * np.sqrt(N) * np.linalg.norm(F["fr"], axis=-1)[:, None]
    return 2.0 * np.abs(F["X"]) * E + E ** 2 + 4.0 * U * F["P"]


def decided(F, N, kappa, guard, static=None):
    """The bins at which any detection within delta of the reference's powers gives the reference's e, by the monotonicity of order
    statistics: a bin is surely detected when P - delta > kappa med(P + delta) (1 + 4 u), surely not when P + delta < kappa
    med(P - delta) (1 - 4 u).  e[f] is decided when it is static, when a surely detected bin lies within the guard, or when every
    bin within the guard is surely not detected.  -> (decided [frames, N], undecided detections [frames, N])"""
    d = power_tolerance(F, N)
    hi = kappa * lower_median(F["P"] + d)[:, None] * (1.0 + 4.0 * U)
    lo = kappa * lower_median(np.maximum(F["P"] - d, 0.0))[:, None] * (1.0 - 4.0 * U)
    on, off = F["P"] - d > hi, F["P"] + d < lo
    unsure = ~(on | off)
    dec = widen(on, guard, static) | ~widen(unsure, guard)
    return dec, unsure
