"""numpy transcription of k_neg.hip's draw: the counter hash and the k-th-missing search."""
import numpy as np

U = np.uint64
GOLD, M1, M2 = U(0x9E3779B97F4A7C15), U(0xBF58476D1CE4E5B9), U(0x94D049BB133111EB)


def mix(z):
    """splitmix64's finaliser over a uint64 array (wrapping)."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * M1
        z = (z ^ (z >> U(27))) * M2
        return z ^ (z >> U(31))


def draw(src, n, excl_ptr, excl_idx, seed, round):
    """dst[e]: the r-th node outside src[e]'s strictly ascending exclusion row."""
    src = np.asarray(src, np.int64)
    with np.errstate(over="ignore"):
        k = mix(np.array([seed], U) + GOLD * U(round + 1))
        h = mix(k + GOLD * (np.arange(len(src), dtype=U) + U(1)))
    dst = np.empty(len(src), np.int32)
    for e, s in enumerate(src):
        x = np.asarray(excl_idx[excl_ptr[s]:excl_ptr[s + 1]], np.int64)
        r = (int(h[e]) >> 32) * (n - len(x)) >> 32
        dst[e] = r + np.searchsorted(x - np.arange(len(x)), r, side="right")
    return dst
