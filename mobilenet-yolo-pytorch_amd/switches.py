"""Every MNY_* environment variable of the project, in one table.

Rows: (name, type, default, reader, meaning).  `reader` says who looks at it: "lib" = libmnyolo.so (the same row is in the MNY_SWITCHES table of
csrc/common.h, read through mny::sw), "plan" = the plan compiler (engine.py, read at the top of NetPlan construction), "loader" = _lib.py,
"bench" = bench.py alone.  tests/test_abi.py holds this table, the C table and every reading site together.

Types: FLAG is on when set to anything but "" or "0"; INT is int(value), the default when unset; WORD / TEXT are the value itself.
The library reads its switches once per process, at its first use of any of them (MNY_EXDW_STATS and MNY_NMS_SMALL: at every call); the plan
compiler reads its own once per plan.  _lib.load() warns about any other MNY_* variable it finds set: a retired or misspelled switch.
"""
import os
import warnings

FLAG, INT, WORD, TEXT = "flag", "int", "word", "text"

TABLE = (
    ("MNY_LIB", TEXT, None, "loader", "path of another libmnyolo.so build to load (A/B on one machine)"),
    ("MNY_HIPGRAPH", FLAG, 0, "plan", "replay training plans through captured hipGraphs"),
    ("MNY_SIDE_STREAM", INT, None, "plan", "weight gradients on a side stream: 0 / 1, unset = up to 48 M input pixels"),
    ("MNY_NO_GATE", FLAG, 0, "plan", "per-pixel gates as separate convs, BatchNorms and a multiply, not fused units"),
    ("MNY_EXDW_K", TEXT, "16,24", "plan", "input widths whose expand + depthwise pairs run as one unit"),
    ("MNY_NO_LR", FLAG, 0, "plan lib", "no low-rank BatchNorm backward of the wide expand units (lrbwd.hip)"),
    ("MNY_NO_LR_S2", FLAG, 0, "plan", "no low-rank BatchNorm backward behind the stride-2 depthwise units"),
    ("MNY_NO_DWFUSE5S2", FLAG, 0, "plan", "5x5 stride-2 depthwise units on the generic backward kernels"),
    ("MNY_GEMM_V1", FLAG, 0, "lib", "pointwise forward / data gradients on the first-generation tile kernels"),
    ("MNY_WGRAD_V1", FLAG, 0, "lib", "pointwise weight gradients on the first-generation tile kernel"),
    ("MNY_WGRAD_NO_XCD", FLAG, 0, "lib", "weight-gradient workgroups in plain order, not grouped per XCD"),
    ("MNY_X6", INT, -1, "lib", "six-product bf16 GEMM: 0 = never (fp32 MFMA), 1 = wherever supported, -1 = per-shape rule"),
    ("MNY_NO_W6", FLAG, 0, "lib", "no pre-cut weight operand for the six-product GEMM"),
    ("MNY_NO_WIDE", FLAG, 0, "lib", "no barrier-free short-reduction kernel (pwwide.hip)"),
    ("MNY_NO_WGS", FLAG, 0, "lib", "no stream weight-gradient kernel (pwwgs.hip)"),
    ("MNY_NO_THIN", FLAG, 0, "lib", "no vector-ALU kernel for K = 8..32 (pwthin.hip)"),
    ("MNY_NO_PWT", FLAG, 0, "lib", "no wave-per-16-pixels thin pointwise kernel (gate.hip)"),
    ("MNY_NO_PWE", FLAG, 0, "lib", "no wave form of the thin expand unit backward (gate.hip)"),
    ("MNY_NO_PJBWD", FLAG, 0, "lib", "no fused projection backward (pjbwd.hip, gate.hip)"),
    ("MNY_NO_EXDW", FLAG, 0, "lib", "no fused expand + depthwise unit: the materialised path"),
    ("MNY_EXDW_STATS", WORD, 0, "lib", "gram (default) | direct: how mny_exdw_stats forms its sums"),
    ("MNY_NO_STEMDW", FLAG, 0, "lib", "no fused stem + depthwise backward (stemdw.hip)"),
    ("MNY_STEM_WGRAD_VALU", FLAG, 0, "lib", "stem weight gradient on the vector ALU, not the matrix cores"),
    ("MNY_DW_V1", FLAG, 0, "lib", "3x3 depthwise forward on the first-generation sliding-window kernel"),
    ("MNY_NO_DWT5", FLAG, 0, "lib", "no tile form of the 5x5 depthwise unit backward"),
    ("MNY_DWT3", INT, -1, "lib", "tile form of the 3x3 depthwise unit backward: 0 / 1, -1 = per-shape rule"),
    ("MNY_DWTF", INT, -1, "lib", "tile form of the depthwise forward: 0 / 1, -1 = per-shape rule"),
    ("MNY_NMS_SMALL", FLAG, 0, "lib", "NMS buckets of any size through the one-workgroup path"),
    ("MNY_FORCE_DP", FLAG, 0, "bench", "bench.py: run the RCCL data-parallel path even with one rank"),
    ("MNY_LAUNCHER_PARENT_CLEAN", FLAG, 0, "bench", "bench.py: set by its launcher for the rank processes it starts"),
    ("MNY_PRINT_MARKS", FLAG, 0, "bench", "bench.py: print the backward call list's marks"),
)
_ROWS = {row[0]: row for row in TABLE}


def get(name):
    """Value of the switch `name` (a row of TABLE; anything else is a KeyError) as the environment has it now."""
    _, kind, default, _, _ = _ROWS[name]
    raw = os.environ.get(name)
    if kind == FLAG:
        return raw not in (None, "", "0")
    if raw in (None, ""):
        return default
    return int(raw) if kind == INT else raw


def warn_unknown():
    """One warning per MNY_* variable of the environment that no row names."""
    for name in sorted(os.environ):
        if name.startswith("MNY_") and name not in _ROWS:
            warnings.warn("%s is set but is not a switch of this build (retired or misspelled?): it has no effect — see switches.py" % name,
                          RuntimeWarning, stacklevel=3)
