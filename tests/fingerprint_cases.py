"""The numpy restatement of csbsr_fingerprint (include/csbsr_hip.h) and the tensor list the device test runs it on.

A tensor is read as n little-endian 32-bit words w_j; with np.uint64 arithmetic, which wraps modulo 2^64 like the kernel's:

    row[0] = sum_j w_j            row[1] = sum_j w_j (j + 1)

The result is returned as int64 (the same bits), which is how csbsr_amd.parallel.agree.fingerprint returns the device's table."""
import numpy as np

WORDS = (1, 3, 8191, 8192, 8193, 20000)          # around the 8192-word chunk of one workgroup, and more than two chunks


def words_of(a):
    """the bytes of a C-contiguous array as uint32 words"""
    a = np.ascontiguousarray(a)
    assert a.nbytes % 4 == 0
    return a.reshape(-1).view(np.uint8).view("<u4")


def fingerprint_numpy(arrays):
    out = np.zeros((len(arrays), 2), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for t, a in enumerate(arrays):
            w = words_of(a).astype(np.uint64)
            j1 = np.arange(1, w.size + 1, dtype=np.uint64)
            out[t, 0] = np.add.reduce(w, dtype=np.uint64)
            out[t, 1] = np.add.reduce(w * j1, dtype=np.uint64)
    return out.view(np.int64)


def host_cases(seed=5):
    """[(name, numpy array)]: fp32 tensors of every size in WORDS (random bits: NaN payloads, infinities and denormals included), int64
    tensors (two words per element; odd and even element counts), an empty tensor, and all-ones words.  The weighted sum of n words of
    0xFFFFFFFF is about 2^32 n^2 / 2: it stays below 2^64 for the 20000-word case (2^59.6) and wraps eight times over for the 2^18-word
    one, so column 1 is compared on both sides of the wrap.  (Column 0 cannot wrap below 2^32 words, 16 GiB of one tensor; its 64-bit
    carries are exercised from 2 words of 0xFFFFFFFF on.)"""
    rng = np.random.default_rng(seed)
    cases = [(f"f32_{n}", rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype("<u4").view(np.float32)) for n in WORDS]
    cases += [(f"i64_{n}", rng.integers(-2 ** 63, 2 ** 63 - 1, size=n, dtype=np.int64)) for n in (1, 4097, 10000)]
    cases.append(("empty", np.zeros(0, dtype=np.float32)))
    cases.append(("ones_20000", np.full(20000, 0xFFFFFFFF, dtype="<u4").view(np.float32)))
    cases.append(("ones_wrap", np.full(1 << 18, 0xFFFFFFFF, dtype="<u4").view(np.float32)))
    cases.append(("i64_minus_one", np.full(9000, -1, dtype=np.int64)))
    return cases
