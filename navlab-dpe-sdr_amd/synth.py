"""Seeded synthetic inputs for the sampleblock->BCM path.

Product-side utility used by bench.py, smoke() and the tests; no oracle dependency.
The C/A generator here is an independent restatement (G2 delay-table form, as in
pygnss correlator.py:474-525) of the LFSR that csrc/ implements in the tap-selector form
(batchcorrscores.cu:117-177); tests cross-check the two.
"""
import numpy as np

F_CA = 1.023e6
F_L1 = 1.57542e9
L_CA = 1023
PRNS_R = [2, 3, 6, 12, 17, 19, 24, 28]          # handoff_params_usrp6.csv:5
PRNS_H = PRNS_R + [1, 5, 10, 25]                # SURVEY.md 8d, K=12

_G2_DELAY = [5, 6, 7, 8, 17, 18, 139, 140, 141, 251, 252, 254, 255, 256, 257, 258, 469, 470, 471,
             472, 473, 474, 509, 512, 513, 514, 515, 516, 859, 860, 861, 862, 863, 950, 947, 948, 950]


def ca_code(prn):
    """+/-1 C/A chips, chip = +1 where G1 xor G2 == 1 (correlator.py:515)."""
    g1 = np.zeros(1023, dtype=np.int64)
    g2 = np.zeros(1023, dtype=np.int64)
    r1 = [1] * 10
    r2 = [1] * 10
    for i in range(1023):
        g1[i] = r1[9]
        g2[i] = r2[9]
        f1 = r1[2] ^ r1[9]
        f2 = r2[1] ^ r2[2] ^ r2[5] ^ r2[7] ^ r2[8] ^ r2[9]
        r1 = [f1] + r1[:9]
        r2 = [f2] + r2[:9]
    g2 = np.roll(g2, _G2_DELAY[prn - 1])
    return np.where((g1 + g2) % 2 == 0, -1, 1).astype(np.int8)


def time_idx(S, fs):
    return np.round(np.arange(S) / fs * 1.0e9) / 1.0e9


def nav_bit_boundary(cp_ela, cp_ref, rc, fc, fs):
    since = (int(cp_ela) - int(cp_ref)) % 20
    return int(np.floor((L_CA * (20 - since) - rc) * (fs / fc))) + 1


def random_channels(seed, K, prns=None):
    """Channel parameters per SURVEY.md 8d: fi~U(-4e3,4e3), rc~U(0,1023), ri~U(0,1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    prns = list(prns) if prns is not None else (PRNS_R if K <= 8 else PRNS_H)[:K]
    fi = rng.uniform(-4e3, 4e3, K)
    fc = F_CA * (1.0 + fi / F_L1)
    rc = rng.uniform(0, L_CA, K)
    ri = rng.uniform(0, 1, K)
    cp = np.full(K, 1000, dtype=np.int32)
    cp_ref = (1000 + rng.integers(0, 20, K)).astype(np.int32)
    return dict(prn=np.array(prns, dtype=np.int32), rc=rc, ri=ri, fc=fc, fi=fi, cp=cp, cp_ref=cp_ref)


def gen_iq(seed, fs, S, ch, amp=48.0, sigma=300.0, dc=(3.0, -2.0), flip=None):
    """One window of interleaved int16 I/Q consistent with channel params `ch`.

    flip[k] = True puts a nav-bit sign change at the predicted boundary sample."""
    rng = np.random.Generator(np.random.PCG64(seed))
    K = len(ch["prn"])
    t = time_idx(S, fs)
    x = np.zeros(S, dtype=np.complex128)
    if flip is None:
        flip = rng.integers(0, 2, K).astype(bool)
    amp = np.broadcast_to(np.asarray(amp, dtype=np.float64), (K,))
    for k in range(K):
        chips = ca_code(int(ch["prn"][k])).astype(np.float64)
        r = chips[np.mod(np.floor(t * ch["fc"][k] + ch["rc"][k]).astype(np.int64), L_CA)]
        nb = nav_bit_boundary(ch["cp"][k], ch["cp_ref"][k], ch["rc"][k], ch["fc"][k], fs)
        d = np.ones(S)
        if flip[k] and 0 < nb < S:
            d[nb:] = -1.0
        x += amp[k] * d * r * np.exp(2j * np.pi * (ch["fi"][k] * t + ch["ri"][k]))
    x += sigma * (rng.standard_normal(S) + 1j * rng.standard_normal(S))
    x += complex(dc[0], dc[1])
    iq = np.empty(2 * S, dtype=np.int16)
    iq[0::2] = np.clip(np.rint(x.real), -32768, 32767).astype(np.int16)
    iq[1::2] = np.clip(np.rint(x.imag), -32768, 32767).astype(np.int16)
    return iq


def gen_iq_record(seed, fs, n_samples, ch, amp=48.0, sigma=300.0, nav_bits=None):
    """One CONTINUOUS record of interleaved int16 I/Q: code and carrier phase run on over any window boundary
    (sample n at t = n / fs: code phase t fc + rc, carrier phase fi t + ri, `ch` as for gen_iq, referred to sample 0) and
    a nav-bit sign every 20 code periods.  nav_bits[k]: +-1 per bit of channel k (drawn from the seed when None);
    bit j of channel k covers the code periods [20 j - ch["cp_ref"][k] % 20, ...), i.e. the first edge falls
    cp_ref % 20 code periods after the start of the code period sample 0 lies in (20 when that is 0; bit 0 is then unused).  No DC offset.
    Returns (iq int16 [2 n_samples], nav_bits list of int8 arrays)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    K = len(ch["prn"])
    n = np.arange(n_samples, dtype=np.float64)
    t = n / fs
    amp = np.broadcast_to(np.asarray(amp, dtype=np.float64), (K,))
    x = np.zeros(n_samples, dtype=np.complex128)
    bits_out = []
    for k in range(K):
        chips = ca_code(int(ch["prn"][k])).astype(np.float64)
        cph = t * ch["fc"][k] + ch["rc"][k]
        ci = np.floor(cph).astype(np.int64)
        period = ci // L_CA                                     # code periods since the one sample 0 lies in
        first_edge = int(ch["cp_ref"][k]) % 20 if "cp_ref" in ch else 0
        bit_idx = (period - first_edge + 20) // 20              # 0 before the first edge
        nb = int(bit_idx.max()) + 1
        if nav_bits is None:
            bits = (2 * rng.integers(0, 2, nb) - 1).astype(np.int8)
        else:
            bits = np.asarray(nav_bits[k], dtype=np.int8)
            assert bits.size >= nb, "channel %d needs %d nav bits" % (k, nb)
        bits_out.append(bits[:nb].copy())
        x += amp[k] * bits[bit_idx] * chips[np.mod(ci, L_CA)] * np.exp(2j * np.pi * (ch["fi"][k] * t + ch["ri"][k]))
    x += sigma * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    iq = np.empty(2 * n_samples, dtype=np.int16)
    iq[0::2] = np.clip(np.rint(x.real), -32768, 32767).astype(np.int16)
    iq[1::2] = np.clip(np.rint(x.imag), -32768, 32767).astype(np.int16)
    return iq, bits_out


def gen_iq_record_chunks(seed, fs, n_samples, ch, nav_bits, amp=48.0, sigma=300.0, chunk=1 << 20):
    """gen_iq_record's record in pieces, so that a record of many seconds needs memory for one piece: yields int16 arrays of
    up to 2 * chunk interleaved I/Q values, in order.  Signal model, `ch` and the nav-bit convention are gen_iq_record's (sample n
    at t = n / fs whatever piece it falls in; nav_bits[k][j] as there, and required: the caller knows how many bits its record
    spans).  The noise of piece i is drawn from PCG64((seed, i)), so the samples depend on `chunk` and are not gen_iq_record's."""
    K = len(ch["prn"])
    amp = np.broadcast_to(np.asarray(amp, dtype=np.float64), (K,))
    chips = [ca_code(int(p)).astype(np.float64) for p in ch["prn"]]
    bits = [np.asarray(b, dtype=np.int8) for b in nav_bits]
    for i, n0 in enumerate(range(0, n_samples, chunk)):
        m = min(chunk, n_samples - n0)
        rng = np.random.Generator(np.random.PCG64([seed, i]))
        t = np.arange(n0, n0 + m, dtype=np.float64) / fs
        x = sigma * (rng.standard_normal(m) + 1j * rng.standard_normal(m))
        for k in range(K):
            ci = np.floor(t * ch["fc"][k] + ch["rc"][k]).astype(np.int64)
            first_edge = int(ch["cp_ref"][k]) % 20 if "cp_ref" in ch else 0
            bit_idx = (ci // L_CA - first_edge + 20) // 20
            assert bit_idx[-1] < bits[k].size, "channel %d needs %d nav bits" % (k, int(bit_idx[-1]) + 1)
            ph = ch["fi"][k] * t + ch["ri"][k]
            x += amp[k] * bits[k][bit_idx] * chips[k][np.mod(ci, L_CA)] * np.exp(2j * np.pi * (ph - np.floor(ph)))
        iq = np.empty(2 * m, dtype=np.int16)
        iq[0::2] = np.clip(np.rint(x.real), -32768, 32767).astype(np.int16)
        iq[1::2] = np.clip(np.rint(x.imag), -32768, 32767).astype(np.int16)
        yield iq


def cn0_to_amp(cn0_dbhz, sigma, fs):
    """Carrier amplitude for a carrier-to-noise-density ratio in dB-Hz: with complex noise of standard deviation sigma per
    component sampled at fs the noise density is N0 = 2 sigma^2 / fs, the carrier power C = amp^2, so C/N0 = amp^2 fs / (2 sigma^2)."""
    return np.sqrt(2.0 * np.square(np.asarray(sigma, dtype=np.float64)) / fs * 10.0 ** (np.asarray(cn0_dbhz, dtype=np.float64) / 10.0))


def amp_to_cn0(amp, sigma, fs):
    """The inverse of cn0_to_amp: C/N0 in dB-Hz of a carrier of amplitude amp."""
    return 10.0 * np.log10(np.square(np.asarray(amp, dtype=np.float64)) * fs / (2.0 * np.square(np.asarray(sigma, dtype=np.float64))))


def rand_grid(seed, G, half=(110.0, 110.0, 110.0, 132.0)):
    """rngrid3-format random ENU-dt grid (SURVEY.md 8d iii): columns x,y,z,delta_t (m)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.uniform(-1.0, 1.0, (G, 4)) * np.asarray(half)[None, :]
    return g


def uniform_grid(dim, spacing):
    """Uniform tensor grid, x slowest / t fastest (batchcorrmanifold.cu:165-182)."""
    half = (dim - 1) // 2
    ax = spacing * (np.arange(dim) - half)
    X, Y, Z, T = np.meshgrid(ax, ax, ax, ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel(), T.ravel()], axis=1)


def spread_grid():
    """PyGNSS spread grids (receiver.py:995-1026): returns (pos[G,4], vel[G,4])."""
    a = np.array([-22, -19, -16, -13, -10, -7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 10, 13,
                  16, 19, 22], dtype=np.float64)
    b = np.arange(-12, 13, dtype=np.float64)
    X, Y, Z, T = np.meshgrid(a * 5, a * 5, a * 5, a * 6, indexing="ij")
    pos = np.stack([X.ravel(), Y.ravel(), Z.ravel(), T.ravel()], axis=1)
    X, Y, Z, T = np.meshgrid(b * 0.5, b * 0.5, b * 0.5, b * 0.25, indexing="ij")
    vel = np.stack([X.ravel(), Y.ravel(), Z.ravel(), T.ravel()], axis=1)
    return pos, vel


def write_grid_csv(path, grid):
    """x,y,z,delta_t per line with CRLF (batchcorrmanifold.cu:2433-2444 loader format)."""
    with open(path, "w", newline="") as f:
        for row in grid:
            f.write("%.17g,%.17g,%.17g,%.17g\r\n" % tuple(row))


def enu2ecef_matrix(p0):
    """Row-major ENU -> ECEF rotation [3, 3] at the ECEF position p0: the arithmetic of csrc/dpe_sat.h's enu2ecef_matrix
    (CHM_Dev_ECEF2LL_Rad + CHM_Dev_R_ENU2ECEF, cuchanmgr.cu:37-73) in numpy."""
    a, b, e, ep = 6378137.0, 6356752.314245, 0.08181919084262149, 0.08209443794969568
    x, y, z = (float(v) for v in np.asarray(p0, dtype=np.float64)[:3])
    p = np.sqrt(x * x + y * y)
    th = np.arctan2(z * a, p * b)
    lat = np.arctan2(z + ep ** 2 * b * np.sin(th) ** 3, p - e ** 2 * a * np.cos(th) ** 3)
    lon = np.arctan2(y, x)
    sa, ca, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    return np.array([[-so, -sa * co, ca * co], [co, -sa * so, ca * so], [0.0, ca, sa]])


def enu_disc_grid(radius_m, step_m, up_m=0.0):
    """Horizontal ENU grid for collective detection: the points of a square lattice of spacing step_m (the origin among them)
    that lie within radius_m of the origin, all at height up_m; rows (east, north, up), east slowest."""
    n = int(np.floor(radius_m / step_m + 1e-9))
    ax = step_m * np.arange(-n, n + 1, dtype=np.float64)
    E, N = np.meshgrid(ax, ax, indexing="ij")
    keep = E * E + N * N <= radius_m * radius_m * (1.0 + 1e-12)
    return np.stack([E[keep], N[keep], np.full(int(keep.sum()), float(up_m))], axis=1)
