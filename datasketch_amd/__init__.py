"""datasketch_amd -- MI355X-native MinHash signature engine with the datasketch API.

Drop-in for the bulk-hashing hot path of ekzhu/datasketch (``MinHash.update_batch`` / ``bulk`` /
``generator`` and ``WeightedMinHashGenerator.minhash_many``): same class names, arguments and
results, with the permutation + min kernels written in HIP for gfx950 and reached through a
ctypes C ABI (``include/mhx.h``).  No PyTorch / CuPy / Triton on the path.
"""
from datasketch_amd.b_bit_minhash import bBitMinHash
from datasketch_amd import lsh_bulk
from datasketch_amd import hyperloglog
from datasketch_amd import shingle
from datasketch_amd import overlap
from datasketch_amd.hashfunc import hash_many, prehashed, sha1_hash32, sha1_hash64, sha1_hash_many, xxh32_hash32, xxh64_hash64
from datasketch_amd.hyperloglog import HyperLogLog
from datasketch_amd.lean_minhash import LeanMinHash
from datasketch_amd.lsh import MinHashLSH
from datasketch_amd.lsh_bloom import BloomTable, MinHashLSHBloom
from datasketch_amd.lshensemble import MinHashLSHEnsemble
from datasketch_amd.lshforest import MinHashLSHForest
from datasketch_amd.minhash import MinHash
from datasketch_amd.weighted_minhash import WeightedMinHash, WeightedMinHashGenerator

__version__ = "0.1.0"

__all__ = [
    "HyperLogLog",
    "LeanMinHash",
    "MinHash",
    "MinHashLSH",
    "MinHashLSHBloom",
    "BloomTable",
    "MinHashLSHEnsemble",
    "MinHashLSHForest",
    "WeightedMinHash",
    "WeightedMinHashGenerator",
    "bBitMinHash",
    "prehashed",
    "sha1_hash32",
    "sha1_hash64",
    "sha1_hash_many",
    "xxh32_hash32",
    "xxh64_hash64",
    "hash_many",
    "hyperloglog",
    "lsh_bulk",
    "shingle",
    "overlap",
]
