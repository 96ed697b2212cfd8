"""The comparisons the channel family's golden and GPU tests share."""
import numpy as np


def same_bytes(a, b):
    """Type, shape and every byte."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def zeros_alike(a):
    """The bytes with every -0 made +0: what 'byte for byte' means where the sign of a zero is not part of the contract."""
    v = np.ascontiguousarray(a).view(np.float32).copy()
    v[v == 0] = 0.0
    return v.tobytes()


def same(a, b):
    """Bit for bit, except that +0 and -0 are the same value."""
    a, b = np.ascontiguousarray(a, np.complex64).view(np.float32), np.ascontiguousarray(b, np.complex64).view(np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))))
