"""Per-pair contacts, the parts that need no GPU: decoding contact words into rows and CSR, and the C ABI of
mjpl_contacts* (declared in include/mjpl_hip.h, exported by the built library, bound by mjpl_amd.engine)."""
import os
import re

import numpy as np
import pytest

from mjpl_amd import build as _build
from mjpl_amd import engine
from mjpl_amd.constraint.collision_constraint import contact_csr, contact_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_contact_pair_count", "mjpl_contact_pairs", "mjpl_contacts", "mjpl_contacts_dev")


def pack(hit: np.ndarray) -> np.ndarray:
    """bool [N, P] -> uint64 [N, W]: bit p % 64 of word p // 64, written one bit at a time."""
    n, P = hit.shape
    W = (P + 63) // 64
    out = np.zeros((n, W), np.uint64)
    for i in range(n):
        for p in range(P):
            if hit[i, p]:
                out[i, p // 64] |= np.uint64(1) << np.uint64(p % 64)
    return out


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 213])
def test_decode_words_to_csr(P):
    rng = np.random.default_rng(P)
    n = 37
    hit = rng.random((n, P)) < 0.1
    hit[3] = False  # a configuration without contacts
    if P:
        hit[5] = True  # ... and one with every pair
    pairs = np.stack([rng.integers(0, 50, P), rng.integers(50, 100, P)], axis=1).astype(np.int32)
    bits = pack(hit)
    assert bits.shape == (n, (P + 63) // 64)
    np.testing.assert_array_equal(contact_hits(bits, P), hit)
    offsets, rows = contact_csr(bits, pairs)
    assert offsets.dtype == np.int64 and offsets.shape == (n + 1,) and offsets[0] == 0
    assert rows.dtype == np.int32 and rows.shape == (int(hit.sum()), 2)
    for i in range(n):
        np.testing.assert_array_equal(rows[offsets[i]:offsets[i + 1]], pairs[np.flatnonzero(hit[i])])


def test_bits_beyond_the_last_pair_are_ignored():
    # P = 65: word 1 carries one pair; whatever else sits in it is no pair
    pairs = np.arange(130, dtype=np.int32).reshape(65, 2)
    bits = np.array([[0, 1 | (1 << 7)], [1 << 63, 0]], np.uint64)
    offsets, rows = contact_csr(bits, pairs)
    assert offsets.tolist() == [0, 1, 2]
    assert rows.tolist() == [[128, 129], [126, 127]]


def test_decode_rejects_a_wrong_word_count():
    with pytest.raises(ValueError):
        contact_csr(np.zeros((4, 1), np.uint64), np.zeros((65, 2), np.int32))
    with pytest.raises(ValueError):
        contact_hits(np.zeros((4, 1), np.uint64), 0)


def test_empty_batch():
    offsets, rows = contact_csr(np.zeros((0, 2), np.uint64), np.zeros((100, 2), np.int32))
    assert offsets.tolist() == [0] and rows.shape == (0, 2)


def test_contact_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), f"{name} is not declared in include/mjpl_hip.h"
        assert name in engine.ABI
    _build.build_hip()
    lib = engine.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by libmjpl_hip.so"
