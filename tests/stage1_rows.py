"""One row per path through stage 1's launches (bcs_launch, csrc/dpe_bcs.hip), each at the smallest shape that reaches it.  Shared by
tests/test_gpu_stage1_forms.py (runs every row on the GPU) and tests/test_bcs_plan_cpu.py (every row is also a row of the plan
table tests/golden/bcs_plan_parent.json, under the same name, so its kernel is checked without a GPU first).

Shapes.  S = 4096 at 2.5 / 5 / 2.046 Msps: 16 sub-tiles of 256 samples, four tiles, two blocks of the wide form's grid.
S = 4352 = 4 passes of 1088 samples at 25 Msps: the smallest window the chip kernels take whole passes of; their create-time
condition (theta chipLen)^2 / 24 < 5e-7 allows B = 1 at C = 65536.  bank16 needs 2048 tiles of 16 sub-tiles: S = 12500 (4 tiles),
8 SVs, 64 windows."""

FUSED = dict(fs=2.5e6, S=4096, K=2, W=1, B=8, kernel="bcs_bank_kernel")
CHIP = dict(fs=25e6, S=4352, K=2, W=1, B=1)

ROWS = [
    dict(FUSED, name="fused-L4", seed=41, L=4),
    dict(FUSED, name="fused-L8", seed=42, L=8),
    dict(FUSED, name="fused-L16", seed=43, L=16),
    dict(FUSED, name="dense-L32", seed=44, L=32),                                  # LH = 32: dense, not fused
    dict(FUSED, name="wide", seed=45, fs=5e6, L=32, env={"DPE_BCS_NO_CHIP": "1"}, kernel="bcs_bank_wide_kernel"),
    dict(FUSED, name="bank16", seed=46, S=12500, K=8, W=64, L=4, kernel="bcs_bank16_kernel"),
    dict(CHIP, name="chip", seed=47, L=31, env={"DPE_BCS_NO_CHIP2": "1"}, kernel="bcs_bank_chip_kernel"),
    dict(CHIP, name="chip2", seed=48, L=31, kernel="bcs_bank_chip2_kernel"),
    dict(CHIP, name="chip2-riding-sums", seed=49, W=3, L=31, env={"DPE_BCS_SUMRIDE_MIN": "2"}, kernel="bcs_bank_chip2_kernel"),
    dict(FUSED, name="dense-L100", seed=50, L=100),                                # five chunks of 65 lags
    dict(CHIP, name="chip-L100", seed=51, L=100, kernel="bcs_bank_chip2_kernel"),  # centre chunk chip2, four side chunks chip
    dict(FUSED, name="forced-fft", seed=52, L=8, env={"DPE_BCS_FORCE_FFT": "1"}, kernel="rocfft full-lag path (bcs_fft_*_kernel)"),
    dict(FUSED, name="graph-capture-and-replay", seed=53, L=8, graph=True),
    dict(FUSED, name="time-table-2-windows", seed=54, fs=2.046e6, K=3, W=2, L=8),
]


def case_of(row):
    from tests import helpers
    return helpers.make_case(seed=row["seed"], fs=row["fs"], S=row["S"], K=row["K"], G=16, W=row["W"])


def run_row(row, case):
    """One handle under the row's switches (read at create), one Update (graph rows: the captures and one replay).
    -> code banks, Doppler banks, read_info(), stage1_kernel."""
    import os

    import torch

    import navlab_dpe_sdr_amd as dpe
    from tests import helpers
    iq, cs, _, _ = helpers.pack_gpu_inputs(case)
    env = row.get("env", {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        bcs = dpe.BatchCorrScores(row["fs"], samples_per_window=row["S"], lag_half_width=row["L"], bin_half_width=row["B"],
                                  max_windows=row["W"], max_channels=row["K"])
        bcs.Start()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    d = torch.from_numpy(iq).to("cuda:0")
    st = None
    if row.get("graph"):
        st = dpe.engine.Stream()
        bcs.set_graph(True)
        torch.cuda.synchronize()
        for _ in range(5):                # one capture per slot of the staging ring (the graph's key names the slot), then a replay
            bcs.Update(d, cs, stream=st)
    else:
        bcs.Update(d, cs)
    code, carr = bcs.read_banks(stream=st)
    info = bcs.read_info(stream=st)
    kernel = bcs.stage1_kernel
    bcs.Stop()
    if st is not None:
        st.close()
    return code.copy(), carr.copy(), info, kernel
