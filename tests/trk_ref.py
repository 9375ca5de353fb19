"""fp64 numpy restatement of the scalar tracking loop (test infrastructure, no GPU, no oracle dependency).

What it restates, operation for operation and in the same order: Receiver.scalar_track (pygnss receiver.py:522-542) =
Correlator.scalar_correlate (scalar/correlator.py:135-283), Channel.scalar_correlation / scalar_time_update /
scalar_measurement_update (scalar/channel.py:104-122, 173-191, 247-273), the DLL / PLL discriminators
(discriminator.py:25-54), the second-order bilinear loop filter (loopfilter.py:37-50, 89-104; filters.py:102-115), the lock
detector (lockdetector.py:64-101) and the SNR meter (snrmeter.py:42-61; filters.py:44-57).  tests/test_trk_cpu.py holds it to
the twin's own logs (fixture O14); the GPU tests use it where no fixture exists (25 Msps) and, with `round_epl`, for the
yardstick "what fp32 correlations cost the reference loop"."""
import math

import numpy as np

import navlab_dpe_sdr_amd as dpe

PI = 3.1415926535898           # constants.py:9 (GPS pi; the twin's wipe-off and PLL discriminator use it)
F_CA, F_L1, L_CA = 1.023e6, 1.57542e9, 1023.0
LOG_NAMES = ("cp", "rc", "ri", "fc", "fi", "iE", "qE", "iP", "qP", "iL", "qL", "dc", "di", "efc", "efi", "dpc", "dpi",
             "fc_bias", "fi_bias", "lock", "lockval", "snr")


def correlate(x, chips, fs, rc, ri, fc, fi, p_a=0j):
    """scalar_correlate on one window x (complex128 [S]).  Returns (e_r, p_r, l_r, cp_compl, signs, p_a_new, case, seg) with
    seg the [3 segments][E, P, L] complex sums (zero where a segment does not exist); case -1 = the twin's fourth branch."""
    S = x.size
    t = np.arange(0, S) / fs
    baseband = x * np.exp(-1j * ((2.0 * PI * fi * t) + (2.0 * PI * ri)))
    fidc = t * fc + rc
    early = chips.take(np.mod(np.floor(fidc + 0.5), L_CA).astype(np.int32))
    prompt = chips.take(np.mod(np.floor(fidc), L_CA).astype(np.int32))
    late = chips.take(np.mod(np.floor(fidc - 0.5), L_CA).astype(np.int32))
    idxs1 = np.floor((L_CA - rc) * (fs / fc)).astype(np.int32) + 1
    idxs2 = np.floor((2.0 * L_CA - rc) * (fs / fc)).astype(np.int32) + 1
    seg = np.zeros((3, 3), dtype=np.complex128)

    def sums(a, b):
        return (np.inner(baseband[a:b], early[a:b]), np.inner(baseband[a:b], prompt[a:b]), np.inner(baseband[a:b], late[a:b]))

    if idxs1 <= S < idxs2:
        e_b, p_b, l_b = sums(None, idxs1)
        e_a, p_a2, l_a = sums(idxs1, None)
        seg[0], seg[1] = (e_b, p_b, l_b), (e_a, p_a2, l_a)
        p_s1 = p_a + p_b
        pos = np.abs(e_b + p_b + l_b + e_a + p_a2 + l_a)
        neg = np.abs(e_b + p_b + l_b - e_a - p_a2 - l_a)
        if pos > neg:
            e_r, p_r, l_r = e_b + e_a, p_b + p_a2, l_b + l_a
        else:
            e_r, p_r, l_r = e_b - e_a, p_b - p_a2, l_b - l_a
        return e_r, p_r, l_r, 1, -np.sign([p_s1.real]), p_a2, 1, seg
    if idxs1 < idxs2 <= S:
        e_b, p_b, l_b = sums(None, idxs1)
        e_s, p_s, l_s = sums(idxs1, idxs2)
        e_a, p_a2, l_a = sums(idxs2, None)
        seg[0], seg[1], seg[2] = (e_b, p_b, l_b), (e_s, p_s, l_s), (e_a, p_a2, l_a)
        p_s1 = p_a + p_b
        pos = np.abs(e_b + p_b + l_b + e_s + p_s + l_s)
        neg = np.abs(e_b + p_b + l_b - e_s - p_s - l_s)
        if pos > neg:
            pos = np.abs(e_s + p_s + l_s + e_a + p_a2 + l_a)
            neg = np.abs(e_s + p_s + l_s - e_a - p_a2 - l_a)
            if pos > neg:
                e_r, p_r, l_r = e_b + e_s + e_a, p_b + p_s + p_a2, l_b + l_s + l_a
            else:
                e_r, p_r, l_r = e_b + e_s - e_a, p_b + p_s - p_a2, l_b + l_s - l_a
        else:
            e_r, p_r, l_r = e_b - e_s - e_a, p_b - p_s - p_a2, l_b - l_s - l_a
        return e_r, p_r, l_r, 2, -np.sign([p_s1.real, p_s.real]), p_a2, 2, seg
    if S < idxs1:
        e_b, p_b, l_b = sums(None, None)
        seg[0] = (e_b, p_b, l_b)
        return e_b, p_b, l_b, 0, np.zeros(0), p_a + p_b, 0, seg
    return None, None, None, 0, np.zeros(0), p_a, -1, seg


class _Bilinear:
    def __init__(self, k):
        self.k, self.h = k, 0

    def update(self, xn):
        h0 = self.h
        self.h = self.h + self.k * xn
        return (self.h + h0) / 2.0


class _Loop:
    def __init__(self, T, Bnp):
        w0p = Bnp / 0.53
        self.Kvp, self.Kpp, self.Kvf = w0p ** 2.0, 1.414 * w0p, 0.0 / 0.25
        self.int = _Bilinear(T)

    def update(self, xp, xf):
        return self.int.update(xp * self.Kvp + xf * self.Kvf) + xp * self.Kpp


class _RunAvg:
    def __init__(self, N):
        self.N, self.average, self.q, self.p = N, 0, [0] * N, 0

    def update(self, xn):
        self.average = self.average + (xn - self.q[self.p]) / self.N
        self.q[self.p] = xn
        self.p = (self.p + 1) % self.N
        return self.average


class _Chan:
    def __init__(self, T):
        self.cloop, self.iloop = _Loop(T, 3.0), _Loop(T, 40.0)
        self.li = self.lq = 0
        self.losscount = self.lockcount = self.lock = 0
        self.mean, self.var, self.avgtime = _RunAvg(20), _RunAvg(20), 20 * T
        self.p_a = 0
        self.cpcount = 0

    def lockdet(self, iP, qP):
        self.li = 0.0247 * abs(iP) + (1 - 0.0247) * self.li
        self.lq = 0.0247 * abs(qP) + (1 - 0.0247) * self.lq
        i, q = self.li / 1.5, self.lq
        if i > q:
            self.losscount = 0
            if self.lockcount > 240:
                self.lock = 1
            else:
                self.lockcount += 1
        else:
            self.lockcount = 0
            if self.losscount > 50:
                self.lock = 0
            else:
                self.losscount += 1
        return self.lock, i - q

    def snr(self, iP, qP):
        z = iP * iP + qP * qP
        z_mean = self.mean.update(z)
        z_var = self.var.update((z - z_mean) ** 2)
        sqrtarg = z_mean * z_mean - z_var
        sqrtarg = sqrtarg if sqrtarg > 0 else 0
        carrier_mean = math.sqrt(sqrtarg)
        noise_var = (z_mean - carrier_mean) / 2
        with np.errstate(all="ignore"):
            logarg = carrier_mean / (2 * self.avgtime * noise_var)
        logarg = logarg if logarg > 1 else 1
        return 10 * math.log10(abs(logarg))


def track(iq, fs, T, prns, init, M, ds=1.0, round_epl=None, first_window=0):
    """Track M windows of `iq` (int16 interleaved, consecutive windows from `first_window`) for `prns`, started from
    init[k] = (rc, ri, fc, fi) by the twin's set_scalar_params.  round_epl: a dtype the six correlator outputs are rounded to
    at every window (np.float32 -> the closed-loop yardstick of tests/test_gpu_trk.py).
    Returns (log {name: [M + 1, K]}, case [M, K], cp_sign list of K arrays, seg [M, K, 3, 3] complex, ps list of K arrays: the
    Re p_s each sign was decided on)."""
    S = int(round(T * fs))
    K = len(prns)
    fcaid = ds * F_CA / F_L1
    chips = [dpe.synth.ca_code(int(p)).astype(np.float64) for p in prns]
    log = {n: np.full((M + 1, K), np.nan) for n in LOG_NAMES}
    case = np.zeros((M, K), dtype=np.int64)
    seg = np.zeros((M, K, 3, 3), dtype=np.complex128)
    signs = [[] for _ in range(K)]
    ps = [[] for _ in range(K)]
    ch = [_Chan(T) for _ in range(K)]
    for k in range(K):
        rc, ri, fc, fi = init[k]
        log["cp"][0, k] = 0
        log["rc"][0, k], log["ri"][0, k], log["fc"][0, k], log["fi"][0, k] = rc, ri, fc, fi
        log["fi_bias"][0, k] = fi
        log["fc_bias"][0, k] = fc - F_CA - fcaid * log["fi_bias"][0, k]
    L = log
    for m in range(M):
        w = iq[2 * S * (first_window + m): 2 * S * (first_window + m + 1)]
        x = w[0::2] + 1j * w[1::2]
        for k in range(K):
            c = ch[k]
            pa_prev = c.p_a
            e_r, p_r, l_r, compl_, sg, c.p_a, case[m, k], seg[m, k] = correlate(x, chips[k], fs, L["rc"][m, k], L["ri"][m, k],
                                                                                L["fc"][m, k], L["fi"][m, k], c.p_a)
            if case[m, k] < 0:
                raise RuntimeError("EXTREME ERROR in scalar correlator: window %d channel %d" % (m, k))
            vals = np.array([e_r.real, e_r.imag, p_r.real, p_r.imag, l_r.real, l_r.imag])
            if round_epl is not None:
                vals = vals.astype(round_epl).astype(np.float64)
            L["iE"][m, k], L["qE"][m, k], L["iP"][m, k], L["qP"][m, k], L["iL"][m, k], L["qL"][m, k] = vals
            L["lock"][m, k], L["lockval"][m, k] = c.lockdet(L["iP"][m, k], L["qP"][m, k])
            L["snr"][m, k] = c.snr(L["iP"][m, k], L["qP"][m, k])
            for j in range(compl_):
                signs[k].append(sg[j])
                ps[k].append((pa_prev + seg[m, k, 0, 1]).real if j == 0 else seg[m, k, 1, 1].real)
                c.cpcount += 1
            # scalar_time_update
            L["rc"][m + 1, k] = np.mod(L["rc"][m, k] + L["fc"][m, k] * T, L_CA)
            L["ri"][m + 1, k] = np.mod(L["ri"][m, k] + L["fi"][m, k] * T, 1.0)
            L["cp"][m + 1, k] = c.cpcount
            for n in ("fc", "fi", "fi_bias", "fc_bias"):
                L[n][m + 1, k] = L[n][m, k]
        mc = m + 1
        for k in range(K):
            c = ch[k]
            iP, qP, iE, qE, iL, qL = (L[n][mc - 1, k] for n in ("iP", "qP", "iE", "qE", "iL", "qL"))
            xp = 0.0
            if iP != 0:
                xp = np.arctan(qP / iP) / (2.0 * PI)
            L["dpi"][mc, k] = xp
            xp = 0.0
            E = np.sqrt(iE ** 2.0 + qE ** 2.0)
            Lt = np.sqrt(iL ** 2.0 + qL ** 2.0)
            if (E + Lt) != 0:
                xp = (E - Lt) / (2.0 * (E + Lt))
            L["dpc"][mc, k] = xp
            L["di"][mc, k] = c.iloop.update(L["dpi"][mc, k], 0.0)
            L["dc"][mc, k] = c.cloop.update(L["dpc"][mc, k], 0.0)
            L["efi"][mc, k] = (L["fi_bias"][mc, k] + L["di"][mc, k]) - L["fi"][mc - 1, k]
            L["efc"][mc, k] = ((F_CA + L["fc_bias"][mc, k] + L["dc"][mc, k]) + fcaid * (L["fi_bias"][mc, k] + L["di"][mc, k])) \
                - L["fc"][mc - 1, k]
            L["fi"][mc, k] = L["fi"][mc - 1, k] + L["efi"][mc, k]
            L["fc"][mc, k] = L["fc"][mc - 1, k] + L["efc"][mc, k]
    return log, case, [np.array(s, dtype=np.float64) for s in signs], seg, [np.array(p) for p in ps]


def o14_iq(g):
    """Fixture O14 keeps its synthesis inputs and a digest of the samples, not the samples: rebuild them and check the digest."""
    import hashlib
    K = len(g["prn"])
    ch = dict(prn=g["prn"], rc=g["syn_rc"], ri=g["syn_ri"], fc=g["syn_fc"], fi=g["syn_fi"], cp_ref=g["syn_cp_ref"])
    bits = [g["nav_bits"][k, :int(g["nav_bits_n"][k])] for k in range(K)]
    iq, _ = dpe.synth.gen_iq_record(int(g["seed"]), float(g["fs"]), int(g["n_samples"]), ch, amp=g["amp"], sigma=float(g["sigma"]))
    assert hashlib.sha256(iq.tobytes()).hexdigest() == str(g["iq_sha256"]), "O14: the rebuilt samples differ from the recorded ones"
    assert all(np.array_equal(b, c) for b, c in zip(bits, _)), "O14: the rebuilt nav bits differ from the recorded ones"
    return iq


def scale(name, g, k):
    """What a residual of log quantity `name` is measured against, per channel: correlations against the median prompt magnitude,
    frequencies against 1 Hz, phases / discriminators / counts / dB absolutely."""
    if name in ("iE", "qE", "iP", "qP", "iL", "qL", "lockval"):
        M = int(g["M"])
        return float(np.median(np.hypot(g["log_iP"][:M, k], g["log_qP"][:M, k])))
    return 1.0


def nav_bit_agreement(signs, bits, cp_ref, skip):
    """Fraction of the cp_sign entries from `skip` on that equal the synthesised nav bits (gen_iq_record).  Entry j is decided at the
    j-th code-period boundary the tracker meets, i.e. on code period j counted from the one sample 0 lies in -- or j + 1 when the
    start code phase lies just across a boundary from the truth; the alignment that fits is taken.  1.0 or 0.0 = the bit stream
    up to the PLL's half-cycle ambiguity (and the twin's minus sign)."""
    best = None
    for o in (0, 1):
        j = np.arange(len(signs)) + o
        b = np.asarray(bits)[(j - cp_ref % 20 + 20) // 20]
        a = float(np.mean(np.asarray(signs)[skip:] == b[skip:]))
        if best is None or abs(a - 0.5) > abs(best - 0.5):
            best = a
    return best
