"""A restatement of the acquisition configurations that tests/test_gpu_acq.py runs, one row each, with the search form its
docstrings claim for them.  The older tests there keep their shapes in their own text, so this list follows them by hand: a
changed test needs its row changed with it (tests/test_acq_plan_cpu.py holds the three fixture rows to the fixtures' own fs, S,
bins and PRNs, the rest to nothing but this list).  The two statistics tests that came with this list take their shapes from here
(STATS_RADIX_LDS, STATS_RADIX_MEMORY).  tests/test_acq_plan_cpu.py: every row is also a row of the plan table
tests/golden/acq_plan_parent.json, under the same name, so the form and the kernels are checked without a GPU first.

A row: fs, S, P PRNs (1 .. P unless `prns` lists them), B bins of `step` Hz centred on 0, mode, prn_chunk, the switches set at
create (env) -> corr / fwd (the names of csrc/dpe_acq_plan.h's two enums), kernels (launches the row must contain) and stats (where
the statistics kernel keeps the row: "registers" = acq_stats_small_kernel, "lds" / "memory" = acq_stats_kernel)."""
import numpy as np


def _row(*parts, **fields):
    row = {}
    for p in parts:
        row.update(p)
    row.update(fields)
    return row


R25 = _row(fs=2.5e6, S=25000, step=100.0, chunk=0, stats="registers")
FUSED = _row(corr="fused-2500", fwd="wipe-fold+rocfft", kernels=["acq_wipe_fold_kernel", "rocfft forward", "acq_corr2500_kernel<false>"])
TEXTBOOK = _row(corr="fused-2500", fwd="acq_wipe_fft2500_kernel", kernels=["acq_wipe_fft2500_kernel", "acq_corr2500_kernel<false>"])
PACKED = _row(corr="alias-packed", fwd="acq_fwd25k_pack_kernel", kernels=["acq_fwd25k_pack_kernel", "acq_corr25k_pack_kernel"])
CHAIN = _row(corr="rocfft-chain", kernels=["rocfft forward", "acq_mul_kernel", "rocfft inverse", "acq_fold_kernel"])
NO_FUSED = {"DPE_ACQ_NO_FUSED": "1"}

ROWS = [
    # test_acq_vs_reference_fixture_and_oracle, test_acq_textbook_mode_vs_oracle (fixture O8: six PRNs)
    _row(R25, FUSED, name="o8-coherent", P=6, B=125, mode="coherent", chunk=4),
    _row(R25, PACKED, name="o8-noncoherent", P=6, B=25, step=500.0, mode="noncoherent", chunk=4),
    _row(R25, TEXTBOOK, name="o8-textbook", P=6, B=25, step=500.0, mode="textbook"),
    # test_acq_32_prns_full_search
    _row(R25, FUSED, name="full-coherent", P=32, B=125, mode="coherent", chunk=32),
    _row(R25, PACKED, name="full-noncoherent-125", P=32, B=125, mode="noncoherent", chunk=32),
    _row(R25, TEXTBOOK, name="full-textbook", P=32, B=125, mode="textbook", chunk=32),
    _row(R25, PACKED, name="full-noncoherent-25", P=32, B=25, step=500.0, mode="noncoherent", chunk=32),
    # test_fused_coherent_search_equals_the_rocfft_chain
    _row(R25, FUSED, name="coherent-fused", P=32, B=125, mode="coherent"),
    _row(R25, CHAIN, name="coherent-rocfft", P=32, B=125, mode="coherent", env=NO_FUSED, fwd="wipe-fold+rocfft"),
    # test_fused_noncoherent_search_equals_the_rocfft_chain
    _row(R25, PACKED, name="noncoherent-fused", P=32, B=25, step=500.0, mode="noncoherent", chunk=32),
    _row(R25, PACKED, name="noncoherent-fused8", P=32, B=25, step=500.0, mode="noncoherent", chunk=8),
    _row(R25, PACKED, name="noncoherent-fused5", P=32, B=25, step=500.0, mode="noncoherent", chunk=5),
    _row(R25, PACKED, name="noncoherent-fused1", P=32, B=25, step=500.0, mode="noncoherent", chunk=1),
    _row(R25, name="noncoherent-rocfft-fwd", P=32, B=25, step=500.0, mode="noncoherent", chunk=32, env={"DPE_ACQ_NO_FWD_PACK": "1"},
         corr="alias-packed", fwd="wipe+rocfft", kernels=["acq_wipe_kernel", "rocfft forward", "acq_decimate10_kernel", "acq_corr25k_pack_kernel"]),
    _row(R25, name="noncoherent-round4", P=32, B=25, step=500.0, mode="noncoherent", chunk=8, env={"DPE_ACQ_NO_PACK": "1"},
         corr="alias-radix10-2500", fwd="wipe+rocfft", kernels=["acq_wipe_kernel", "rocfft forward", "acq_radix10_kernel", "acq_corr2500_kernel<true>"]),
    _row(R25, CHAIN, name="noncoherent-rocfft", P=32, B=25, step=500.0, mode="noncoherent", chunk=8, env=NO_FUSED, fwd="wipe+rocfft"),
    # test_acq_statistics_with_a_long_delay_row, test_acq_statistics_of_a_nearly_constant_row
    _row(CHAIN, name="long-delay-row", fs=16.368e6, S=16368, prns=[6, 21, 13], P=3, B=17, step=500.0, mode="coherent", chunk=0,
         fwd="wipe-fold+rocfft", stats="memory"),
    _row(R25, FUSED, name="nearly-constant-row", prns=[1, 9, 30], P=3, B=9, mode="coherent"),
    # test_o9_fine_frequency_and_two_window_driver (fixture O9: six PRNs)
    _row(R25, FUSED, name="o9-search-signal", prns=[3, 11, 22, 31, 7, 26], P=6, B=125, mode="coherent"),
]

# test_fused_search_at_4_and_5_msps (32 PRNs x 31 bins, chunks of 8, fused and DPE_ACQ_NO_FUSED=1), test_search_signal_at_4_and_5_msps
for _M in (4000, 5000):
    _rate = _row(fs=_M * 1e3, S=10 * _M, P=32, B=31, chunk=8, stats="lds")
    _mixed = "acq_corr_mixed_kernel<%d, 10, %d, 5, %%s>" % (_M, 8 if _M == 4000 else 10)
    ROWS += [
        _row(_rate, name="%d-coherent-fused" % _M, step=100.0, mode="coherent", corr="fused-mixed", fwd="wipe-fold+rocfft",
             kernels=["acq_wipe_fold_kernel", _mixed % "false"]),
        _row(_rate, name="%d-textbook-fused" % _M, step=500.0, mode="textbook", corr="fused-mixed", fwd="wipe+rocfft",
             kernels=["acq_wipe_kernel", _mixed % "false"]),
        _row(_rate, name="%d-noncoherent-fused" % _M, step=500.0, mode="noncoherent", corr="alias-radix10-mixed", fwd="wipe+rocfft",
             kernels=["acq_wipe_kernel", "acq_radix10_kernel", _mixed % "true"]),
        _row(_rate, CHAIN, name="%d-coherent-rocfft" % _M, step=100.0, mode="coherent", env=NO_FUSED, fwd="wipe-fold+rocfft"),
        _row(_rate, CHAIN, name="%d-textbook-rocfft" % _M, step=500.0, mode="textbook", env=NO_FUSED, fwd="wipe+rocfft"),
        _row(_rate, CHAIN, name="%d-noncoherent-rocfft" % _M, step=500.0, mode="noncoherent", env=NO_FUSED, fwd="wipe+rocfft"),
        _row(_rate, name="%d-search-signal" % _M, P=4, prns=[5, 14, 23, 9], B=41, step=100.0, chunk=0, mode="coherent", corr="fused-mixed",
             fwd="wipe-fold+rocfft", kernels=["acq_wipe_fold_kernel", _mixed % "false"]),
    ]

# The radix fallback of the statistics through the walked row (tests/test_gpu_acq.py): a DC window, coherent mode, PRNs 1 and 30
STATS_RADIX_LDS = _row(name="stats-radix-row-in-lds", fs=4.0e6, S=40000, prns=[1, 30], P=2, B=9, step=100.0, mode="coherent", chunk=0,
                       corr="fused-mixed", fwd="wipe-fold+rocfft", kernels=["acq_corr_mixed_kernel<4000, 10, 8, 5, false>", "acq_stats_kernel"],
                       stats="lds")
STATS_RADIX_MEMORY = _row(CHAIN, name="stats-radix-row-in-memory", fs=12.0e6, S=120000, prns=[1, 30], P=2, B=5, step=100.0, mode="coherent",
                          chunk=0, fwd="wipe-fold+rocfft", stats="memory")
ROWS += [STATS_RADIX_LDS, STATS_RADIX_MEMORY]
for _r in ROWS:
    _r["kernels"] = _r["kernels"] + ["acq_stats_small_kernel" if _r["stats"] == "registers" else "acq_stats_kernel"]


def prns_of(row):
    return list(row.get("prns", range(1, row["P"] + 1)))


def bins_of(row):
    return (np.arange(row["B"]) - row["B"] // 2) * row["step"]


def dc_window(S, seed=5):
    """I + 1000, Q - 300 and +-1 LSB of noise: every delay of the 0 Hz bin correlates alike (DC x the code's chip sum), so the
    values of max_percode differ by a few percent and crowd into a few of the statistics' bins of width mean / 256."""
    iq = np.random.default_rng(seed).integers(-1, 2, size=2 * S).astype(np.int16)
    iq[0::2] += 1000
    iq[1::2] -= 300
    return iq


def create(row):
    """An Acquisition under the row's switches (read at create)."""
    import os

    import navlab_dpe_sdr_amd as dpe
    env = row.get("env", {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return dpe.Acquisition(row["fs"], row["S"], prns_of(row), bins_of(row), mode=row["mode"], prn_chunk=row["chunk"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
