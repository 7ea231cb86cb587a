"""Token hash functions.

The reference hashes tokens in Python on the CPU and hands integers to the permutation step
(datasketch/hashfunc.py:5-28, datasketch/minhash.py:262-263); these callables are that boundary,
unchanged.  The bulk paths recognise the function objects ``sha1_hash32`` / ``sha1_hash64`` (the
reference's default) and, with a device back end, hash whole chunks of byte tokens with the SHA-1
kernel of libmhx instead of calling them per token (``sha1_hash_many``); results are identical.

``xxh32_hash32`` / ``xxh64_hash64`` are not in the reference: XXH32 and XXH64 with seed 0, written here from the published
algorithm (github.com/Cyan4973/xxHash, doc/xxhash_spec.md) with no dependency on the ``xxhash`` package, whose
``xxh32_intdigest`` / ``xxh64_intdigest`` they equal.  These two functions ARE the definition of the device's second hash family
(csrc/xxh_kernels.hip): the bulk paths recognise the function objects wherever they recognise the SHA-1 pair
(:func:`device_hash`) and hash in place with a few dozen instructions per token where SHA-1 takes nine hundred.
"""
import hashlib
import struct

_U32 = struct.Struct("<I")
_U64 = struct.Struct("<Q")


def sha1_hash32(data):
    """First 4 bytes of SHA1(data) as a little-endian unsigned 32-bit integer
    (same function as the reference's ``datasketch.hashfunc.sha1_hash32``)."""
    return _U32.unpack_from(hashlib.sha1(data).digest())[0]


def sha1_hash64(data):
    """First 8 bytes of SHA1(data) as a little-endian unsigned 64-bit integer
    (same function as the reference's ``datasketch.hashfunc.sha1_hash64``)."""
    return _U64.unpack_from(hashlib.sha1(data).digest())[0]


def prehashed(value):
    """Identity hash function for tokens that already are hash values (non-negative integers < 2**64).

    Semantically the same as the ``fake_hash_func`` idiom of the reference's tests
    (test/utils.py:4-6).  The bulk entry points recognise this exact function object and skip the
    per-token Python call: a numpy integer array (or a ``(values, offsets)`` CSR pair) is then
    handed to the device as is.
    """
    return value


def sha1_hash_many(tokens, bits: int = 32, gpu_mode: str = "detect"):
    """``[sha1_hash32(t) for t in tokens]`` (``bits=64``: ``sha1_hash64``) as a numpy array; on the
    device when one is available (``gpu_mode`` as for MinHash), else with hashlib."""
    import numpy as np

    from datasketch_amd import _native

    if bits not in (32, 64):
        raise ValueError("bits must be 32 or 64")
    tokens = tokens if isinstance(tokens, (list, tuple)) else list(tokens)
    use_gpu = gpu_mode == "always" or (gpu_mode == "detect" and _native.gpu_detected())
    if gpu_mode == "always" and not _native.gpu_available():
        raise RuntimeError("GPU mode 'always' requested but no MI355X / libmhx.so is available.")
    if not use_gpu:
        f = sha1_hash32 if bits == 32 else sha1_hash64
        return np.array([f(t) for t in tokens], dtype=np.uint32 if bits == 32 else np.uint64)
    buf, offsets = _native.Context.pack_tokens(tokens)
    return _native.context().sha1_tokens(buf, offsets, bits)


# ---- xxHash (seed 0) ------------------------------------------------------------------------------------------------------
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
_P32_1, _P32_2, _P32_3, _P32_4, _P32_5 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1
_P64_1, _P64_2, _P64_3, _P64_4, _P64_5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                                          0x27D4EB2F165667C5)
_STRIPE32 = struct.Struct("<4I")
_STRIPE64 = struct.Struct("<4Q")


def _rotl32(x, n):
    return ((x << n) | (x >> (32 - n))) & _M32


def _rotl64(x, n):
    return ((x << n) | (x >> (64 - n))) & _M64


def _round32(acc, w):
    return (_rotl32((acc + w * _P32_2) & _M32, 13) * _P32_1) & _M32


def _round64(acc, w):
    return (_rotl64((acc + w * _P64_2) & _M64, 31) * _P64_1) & _M64


def xxh32_hash32(data):
    """XXH32 of ``data`` with seed 0 as an unsigned 32-bit integer (``xxhash.xxh32_intdigest(data)``)."""
    data = bytes(data)
    n, i = len(data), 0
    if n >= 16:
        v1, v2, v3, v4 = (_P32_1 + _P32_2) & _M32, _P32_2, 0, (-_P32_1) & _M32
        while i + 16 <= n:
            a, b, c, d = _STRIPE32.unpack_from(data, i)
            v1, v2, v3, v4 = _round32(v1, a), _round32(v2, b), _round32(v3, c), _round32(v4, d)
            i += 16
        h = (_rotl32(v1, 1) + _rotl32(v2, 7) + _rotl32(v3, 12) + _rotl32(v4, 18)) & _M32
    else:
        h = _P32_5
    h = (h + n) & _M32
    while i + 4 <= n:
        h = (_rotl32((h + _U32.unpack_from(data, i)[0] * _P32_3) & _M32, 17) * _P32_4) & _M32
        i += 4
    while i < n:
        h = (_rotl32((h + data[i] * _P32_5) & _M32, 11) * _P32_1) & _M32
        i += 1
    h ^= h >> 15
    h = (h * _P32_2) & _M32
    h ^= h >> 13
    h = (h * _P32_3) & _M32
    return h ^ (h >> 16)


def xxh64_hash64(data):
    """XXH64 of ``data`` with seed 0 as an unsigned 64-bit integer (``xxhash.xxh64_intdigest(data)``)."""
    data = bytes(data)
    n, i = len(data), 0
    if n >= 32:
        v1, v2, v3, v4 = (_P64_1 + _P64_2) & _M64, _P64_2, 0, (-_P64_1) & _M64
        while i + 32 <= n:
            a, b, c, d = _STRIPE64.unpack_from(data, i)
            v1, v2, v3, v4 = _round64(v1, a), _round64(v2, b), _round64(v3, c), _round64(v4, d)
            i += 32
        h = (_rotl64(v1, 1) + _rotl64(v2, 7) + _rotl64(v3, 12) + _rotl64(v4, 18)) & _M64
        for v in (v1, v2, v3, v4):
            h = ((h ^ _round64(0, v)) * _P64_1 + _P64_4) & _M64
    else:
        h = _P64_5
    h = (h + n) & _M64
    while i + 8 <= n:
        h = (_rotl64(h ^ _round64(0, _U64.unpack_from(data, i)[0]), 27) * _P64_1 + _P64_4) & _M64
        i += 8
    if i + 4 <= n:
        h = (_rotl64(h ^ ((_U32.unpack_from(data, i)[0] * _P64_1) & _M64), 23) * _P64_2 + _P64_3) & _M64
        i += 4
    while i < n:
        h = (_rotl64(h ^ ((data[i] * _P64_5) & _M64), 11) * _P64_1) & _M64
        i += 1
    h ^= h >> 33
    h = (h * _P64_2) & _M64
    h ^= h >> 29
    h = (h * _P64_3) & _M64
    return h ^ (h >> 32)


# the hash families of libmhx (include/mhx.h: MHX_HASH_SHA1, MHX_HASH_XXH)
HASH_SHA1, HASH_XXH = 0, 1
_DEVICE_HASHES = ((sha1_hash32, (HASH_SHA1, 32)), (sha1_hash64, (HASH_SHA1, 64)), (xxh32_hash32, (HASH_XXH, 32)),
                  (xxh64_hash64, (HASH_XXH, 64)))


def device_hash(hashfunc):
    """``(hash_kind, bits)`` when ``hashfunc`` is one of the four function objects the device hashes in place --
    ``sha1_hash32``, ``sha1_hash64``, ``xxh32_hash32``, ``xxh64_hash64`` -- else ``None``: the one place the bulk paths ask."""
    for f, known in _DEVICE_HASHES:
        if hashfunc is f:
            return known
    return None


def hash_function(kind: int, bits: int):
    """The function object that :func:`device_hash` maps to ``(kind, bits)``."""
    for f, known in _DEVICE_HASHES:
        if known == (kind, bits):
            return f
    raise ValueError("no device hash of kind %r with %r bits" % (kind, bits))


def hash_many(tokens, hashfunc, gpu_mode: str = "detect"):
    """``[hashfunc(t) for t in tokens]`` as a numpy array (uint32 for the two 32-bit device hashes, else uint64); on the device
    when one is available (``gpu_mode`` as for MinHash) and ``hashfunc`` is one of the four of :func:`device_hash`, else per token
    on the host."""
    import numpy as np

    from datasketch_amd import _native

    if gpu_mode not in ("detect", "always", "disable"):
        raise ValueError("gpu_mode must be 'detect', 'always' or 'disable'")
    if not callable(hashfunc):
        raise ValueError("The hashfunc must be a callable.")
    tokens = tokens if isinstance(tokens, (list, tuple)) else list(tokens)
    known = device_hash(hashfunc)
    if gpu_mode == "always" and not _native.gpu_available():
        raise RuntimeError("GPU mode 'always' requested but no MI355X / libmhx.so is available.")
    use_gpu = known is not None and (gpu_mode == "always" or (gpu_mode == "detect" and _native.gpu_detected()))
    if not use_gpu:
        return np.array([hashfunc(t) for t in tokens], dtype=np.uint32 if known and known[1] == 32 else np.uint64)
    buf, offsets = _native.Context.pack_tokens(tokens)
    return _native.context().hash_tokens(buf, offsets, known[1], known[0])
