"""navlab-dpe-sdr_amd -- MI355X-native DPE correlator engine (sampleblock -> BCS -> BCM hot path).

Python side = thin ctypes host layer over the C-ABI in csrc/ (include/dpe_hip.h), plus
synthetic-input and file-format utilities.  Imported as `navlab_dpe_sdr_amd` through the
root-level shim navlab_dpe_sdr_amd.py (the directory name carries a hyphen).
"""
from . import engine, frontend, grid_axes, handoff, pipeline, rinex, sharding, synth, workload  # noqa: F401
from .grid_axes import GridAxes  # noqa: F401
from .engine import Acquisition, ArrayCombiner, BatchCorrManifold, BatchCorrScores, ChanMgr, CollectiveDetector, DpeError, EpochManifold, Excisor, FrontEnd, JointManifold, Pipe, RefineManifold, SubsetManifold, ScalarNavigator, ScalarTracker, Synthesizer, VectorTracker, cuEKF  # noqa: F401

__all__ = ["engine", "frontend", "grid_axes", "GridAxes", "handoff", "pipeline", "rinex", "sharding", "synth", "workload", "BatchCorrScores", "BatchCorrManifold", "JointManifold", "EpochManifold", "SubsetManifold", "RefineManifold", "ChanMgr", "Acquisition", "ScalarTracker", "ScalarNavigator", "VectorTracker", "Synthesizer", "CollectiveDetector", "FrontEnd", "Excisor", "ArrayCombiner", "DpeError", "cuEKF"]
