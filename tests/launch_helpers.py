"""Shared by the GPU tests that look at WHICH kernels ran and under which tune switches (test_gpu_ops_exact.py,
test_gpu_bwd_fused_exact.py, test_gpu_bwd16_fuse.py) and by scripts/executor_fingerprint.py."""
import contextlib
import ctypes as C


def profiled(fn, keep=None, slots=256):
    """Run fn under the library's launch profile (room for `slots` kernel names): (result, {kernel name: launches}).
    keep: only the names that start with one of these prefixes, and never the weight-gradient slab reduce."""
    from flair_amd import _lib as L
    L.check(L.lib().flair_profile_start(slots))
    try:
        res = fn()
    finally:
        n = L.lib().flair_profile_stop()
    assert n >= 0, n
    out = {}
    for i in range(n):
        name = C.create_string_buffer(96)
        ms, cnt, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        L.check(L.lib().flair_profile_kernel(i, name, 96, C.byref(ms), C.byref(cnt), C.byref(fl), C.byref(by)))
        k = name.value.decode()
        if keep is None or (k.startswith(keep) and k != "wgrad_reduce"):
            out[k] = cnt.value
    return res, out


@contextlib.contextmanager
def tuned(pairs, defaults):
    """Set the (key, value) pairs through flair_tune_set; on the way out every key of `defaults` goes back to its default."""
    from flair_amd import _lib as L
    try:
        for k, v in pairs:
            L.check(L.lib().flair_tune_set(k.encode(), v), "flair_tune_set")
        yield
    finally:
        for k, v in defaults.items():
            L.lib().flair_tune_set(k.encode(), v)
