"""Reader for the PyGNSS->CUDARecv handoff CSV (demofiles/handoff_params_usrp6.csv).

Keys and meaning follow DPInit::ParseField (cudarecv/modules/src/dpinit.cpp:247-400) and the
writer pygnss/pythonreceiver/receiver.py:804-875.  Rows: key,v0,v1,...; per-PRN rows are in
prn_list order.  Ephemeris rows (T_GD ... C_is) are the broadcast ephemeris PyGNSS decoded.
"""
import numpy as np

EPH_FIELDS = ["sqrt_A", "e", "i_0", "OMEGA_0", "omega", "M_0", "delta_n", "OMEGADOT", "IDOT",
              "C_rc", "C_rs", "C_uc", "C_us", "C_ic", "C_is", "t_oe", "t_oc",
              "a_f0", "a_f1", "a_f2", "T_GD"]


def read_handoff(path, rinex_path=None):
    """Handoff CSV -> dict.  rinex_path: take the ephemerides from a RINEX nav file instead of the handoff rows, chosen
    as the reference does (DPInit + cuChanMgr, see rinex.py)."""
    rows = {}
    with open(path, "r") as f:
        for line in f:
            parts = line.strip().split(",")
            if len(parts) < 2:
                continue
            rows[parts[0]] = parts[1:]
    out = {
        "rxTime": float(rows["rxTime"][0]),
        "rxTime_a": float(rows["rxTime_a"][0]),
        "X_ECEF": np.array([float(v) for v in rows["X_ECEF"]]),
        "bytes_read": int(rows["bytes_read"][0]),
        "prn_list": np.array([int(v) for v in rows["prn_list"]], dtype=np.int32),
    }
    for k in ("rc", "ri", "fc", "fi"):
        out[k] = np.array([float(v) for v in rows[k]])
    out["cp"] = np.array([int(float(v)) for v in rows["cp"]], dtype=np.int32)
    out["cp_timestamp"] = np.array([int(float(v)) for v in rows["cp_timestamp"]], dtype=np.int32)
    out["TOW"] = np.array([int(float(v)) for v in rows["TOW"]], dtype=np.int32)
    K = out["prn_list"].size
    if rinex_path is not None:
        from . import rinex
        out["eph"] = rinex.select_ephemerides(rinex.read_rinex_nav(rinex_path), out["prn_list"], out["rxTime"])
        return out
    eph = np.zeros((K, len(EPH_FIELDS)))
    for j, name in enumerate(EPH_FIELDS):
        eph[:, j] = [float(v) for v in rows[name]]
    out["eph"] = eph
    return out


# Ephemerides' rows in the order of the shipped file (the twin writes them in the order of a Python 2 dict of ephemeris.py:210-219's
# names; DPInit::ParseField looks rows up by key).  The names read_handoff does not parse are written when the dict carries them.
_EPH_ROW_ORDER = ["T_GD", "C_uc", "t_oe", "t_oc", "total", "complete", "C_rs", "OMEGA_0", "health", "C_rc", "accuracy", "a_f2", "a_f0",
                  "a_f1", "weeknumber", "C_us", "sqrt_A", "OMEGADOT", "M_0", "omega", "i_0", "e", "IDOT", "C_ic", "IODE", "delta_n",
                  "IODC", "C_is"]
_INT_ROWS = ("t_oe", "t_oc")


def _num(v):
    """A number as the twin's csv.writer leaves it: repr of a float (shortest form that reads back to the same double), plain ints."""
    if isinstance(v, (bool, np.bool_)):
        return str(bool(v))
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    return repr(float(v))


def write_handoff(path, ho):
    """dict (read_handoff's form) -> handoff CSV, rows in Receiver.save_scalar_handoff's order (receiver.py:804-875): rxTime,
    rxTime_a, X_ECEF, bytes_read, prn_list, rc, ri, fc, fi, cp, cp_timestamp, TOW, then one row per ephemeris name.  cp is written
    as the float the twin's log holds, t_oe / t_oc as the integers its decode leaves.  Returns path."""
    K = len(ho["prn_list"])
    eph = np.asarray(ho["eph"], dtype=np.float64)
    assert eph.shape == (K, len(EPH_FIELDS))
    rows = [["rxTime", _num(float(ho["rxTime"]))], ["rxTime_a", _num(float(ho["rxTime_a"]))],
            ["X_ECEF"] + [_num(float(v)) for v in np.asarray(ho["X_ECEF"]).ravel()],
            ["bytes_read", _num(int(ho["bytes_read"]))],
            ["prn_list"] + [_num(int(v)) for v in ho["prn_list"]]]
    for k in ("rc", "ri", "fc", "fi"):
        rows.append([k] + [_num(float(v)) for v in ho[k]])
    rows.append(["cp"] + [_num(float(v)) for v in ho["cp"]])
    rows.append(["cp_timestamp"] + [_num(int(v)) for v in ho["cp_timestamp"]])
    rows.append(["TOW"] + [_num(int(v)) for v in ho["TOW"]])
    for name in _EPH_ROW_ORDER:
        if name in EPH_FIELDS:
            col = eph[:, EPH_FIELDS.index(name)]
            if name in _INT_ROWS and np.all(col == np.round(col)):
                rows.append([name] + [_num(int(v)) for v in col])
            else:
                rows.append([name] + [_num(float(v)) for v in col])
        elif name in ho:
            rows.append([name] + [_num(v) for v in np.atleast_1d(ho[name])])
    with open(path, "w", newline="") as f:
        for r in rows:
            f.write(",".join(r) + "\n")
    return path
