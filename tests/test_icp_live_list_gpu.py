"""The live list of a rebuild pass's close, from a wave scan (GPU).

csrc/icp/live_list.h turns the live mask into the ascending list of live chunks: every thread counts the bits of its
mask words, a scan inside each wave and the waves' totals through LDS give it its position, and it expands its words
from there.  pedp_debug_live_list runs that function in one workgroup on mask words of the caller's, with the thread
count, the LDS capacity and the kind of load of the close that uses it at that size: 512 (inside a pass launch; 2,048
entries in LDS) and 1,024 (icp_finish_kernel; 8,192).  The reference is numpy: np.nonzero of the unpacked bits.  The count
and the list are compared byte for byte, and the list's entries behind the count must be untouched.

Word counts: one word; the sizes around a wave (63, 64, 65) and around the thread counts (511, 512, 513; 1025); 1025,
2049 and 3000 give more than one word per thread with 512 and with 1,024 threads.  The mask with more than 8,192 set bits
(beyond both LDS capacities: the list goes to memory alone) exists from 129 words on; below that the full mask is the
densest there is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LW = [1, 2, 63, 64, 65, 511, 512, 513, 1025, 2049, 3000]
PATTERNS = ["empty", "full", "first_bit", "last_top_bit", "random_0.01", "random_0.1", "random_0.5", "over_8192"]
CASES = [(n, p) for n in N_LW for p in PATTERNS if p != "over_8192" or 64 * n > 8192]


def _mask(n_lw, pattern):
    words = np.zeros(n_lw, np.uint64)
    if pattern == "full":
        words[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    elif pattern == "first_bit":
        words[0] = np.uint64(1)
    elif pattern == "last_top_bit":
        words[-1] = np.uint64(1) << np.uint64(63)
    elif pattern.startswith("random") or pattern == "over_8192":
        density = 0.6 if pattern == "over_8192" else float(pattern.split("_")[1])
        rng = np.random.default_rng(1000 * n_lw + PATTERNS.index(pattern))
        bits = (rng.random(64 * n_lw) < density).astype(np.uint8)
        words = np.packbits(bits, bitorder="little").view(np.uint64).copy()
    return words


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("n_lw,pattern", CASES)
def test_live_list_equals_numpy(ctx, threads, n_lw, pattern):
    from pedp_hip import _lib

    words = _mask(n_lw, pattern)
    want = np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))[0].astype(np.int32)
    if pattern == "over_8192":
        assert len(want) > 8192
    n_live, lst = _lib.debug_live_list(ctx, words, threads=threads)
    assert n_live == len(want)
    assert lst.dtype == np.int32 and len(lst) == 64 * n_lw
    assert lst[:n_live].tobytes() == want.tobytes()
    assert (lst[n_live:] == -1).all()
