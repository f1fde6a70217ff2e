"""A digest of a net spec and its images, for the tests that pin a case list against a recorded state: every op dict
key by key in sorted order, arrays as dtype, shape and bytes, everything else as its repr.  Plain numpy."""
import hashlib

import numpy as np


def _feed(h, v):
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        h.update(("array %s %s " % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    elif isinstance(v, (tuple, list)):
        h.update(("%s %d [" % (type(v).__name__, len(v))).encode())
        for e in v:
            _feed(h, e)
        h.update(b"]")
    elif isinstance(v, (np.integer, np.floating, np.bool_)):
        h.update(("%s %r " % (type(v).__name__, v.item())).encode())
    else:
        h.update(("%s %r " % (type(v).__name__, v)).encode())


def array_digest(a):
    h = hashlib.sha256()
    _feed(h, np.asarray(a))
    return h.hexdigest()


def spec_digest(spec, x):
    """sha256 over the images and every op: kernels, biases, BN constants and the rest of each op dict."""
    h = hashlib.sha256()
    _feed(h, np.asarray(x))
    for op in spec:
        h.update(b"op{")
        for k in sorted(op):
            h.update(k.encode() + b"=")
            _feed(h, op[k])
        h.update(b"}")
    return h.hexdigest()
