"""Per-robot rows (srbd.model_rows, a1qp.body_rows, qp.force_body_rows): the
host-side rules the three row types share, stated once."""
import ctypes as C

import numpy as np


def build_rows(batch, length, dtype, columns, fill, overrides, who, prepare=None):
    """A (B, length) host array filled by fill(B, rows), then whole fields
    overwritten by name from `overrides`.  `columns`: field -> (first,
    past-the-last) column.  A value is a scalar, the field's own vector, or a
    per-robot array, (B,) for a width-1 field and (B, width) otherwise;
    prepare(name, array, width), if given, reshapes it first."""
    B = int(batch)
    rows = np.zeros((B, length), dtype)
    fill(B, rows)
    for name, v in overrides.items():
        if name not in columns:
            raise ValueError("%s: unknown field %r (one of %s)" % (who, name, sorted(columns)))
        lo, hi = columns[name]
        a = np.asarray(v, dtype=dtype)
        if prepare is not None:
            a = prepare(name, a, hi - lo)
        if a.ndim == 1 and hi - lo == 1:
            a = a.reshape(-1, 1)          # (B,) of a width-1 field
        rows[:, lo:hi] = np.broadcast_to(a, (B, hi - lo))
    return rows


def rows_from_srbd(model_rows, mapping):
    """Columns of srbd.model_rows rows, widened exactly to float64, as keywords
    for another builder: `mapping` is its field -> the model column's name."""
    from .srbd import MODEL_COLUMNS
    m = np.asarray(model_rows)
    if m.ndim != 2 or m.shape[1] != 16 or m.dtype != np.float32:
        raise ValueError("model_rows: a (B, 16) float32 array of srbd.model_rows expected")
    return {k: m[:, MODEL_COLUMNS[src][0]].astype(np.float64) for k, src in mapping.items()}


def check_row(row, length, ctype, abi_check, message):
    """One row through the C ABI's row rule; ValueError with message()."""
    r = np.ascontiguousarray(row, np.float64)
    if r.shape != (length,):
        raise ValueError("row: %d doubles expected" % length)
    if abi_check(r.ctypes.data_as(C.POINTER(ctype))) != 0:
        raise ValueError(message())


def rows_arg(t, batch, length, dtype, like_device, name="body"):
    """The rows argument of a solve: None, or a contiguous (batch, length)
    `dtype` tensor on `like_device`, a GPU; else ValueError, before a pointer
    reaches the C ABI."""
    import torch
    if t is not None and (
            not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda
            or t.device != like_device or tuple(t.shape) != (batch, length)):
        raise ValueError("%s: a contiguous (%d, %d) %s device tensor on %s expected"
                         % (name, batch, length, dtype, like_device))
    return t
