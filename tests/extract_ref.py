"""gsm_global_extract, gsm_global_state_histogram and the keep-set helpers (include/gsm_renderer.h)
restated in numpy: a boolean index by keep[state] truncated to the capacity, and np.bincount."""
import numpy as np


def keep_bits(keep):
    """the 8 words of a keep set -> 256 booleans, one per state value"""
    w = np.asarray([int(k) & 0xFFFFFFFF for k in keep], np.uint64)
    s = np.arange(256)
    return ((w[s >> 5] >> (s & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)


def keep_words(bits):
    """256 booleans -> the 8 words"""
    bits = np.asarray(bits, bool)
    return [int(sum(1 << b for b in range(32) if bits[32 * k + b])) for k in range(8)]


def keep_visible(hidden):
    """hidden: the `hidden` bytes of a style table (None or empty: no table).  A table past 256 entries is read as
    its first 256."""
    bits = np.ones(256, bool)
    if hidden is not None:
        h = np.asarray(hidden)[:256]
        bits[:len(h)] = h == 0
    return keep_words(bits)


def keep_masked(test_mask, test_value):
    s = np.arange(256)
    return keep_words((s & test_mask & 0xFF) == (test_value & 0xFF))


def states_of(state, count):
    """state: a uint8 array (its first `count` bytes) or an int (every gaussian's state)"""
    if isinstance(state, (int, np.integer)):
        return np.full(count, int(state), np.uint8)
    return np.asarray(state, np.uint8)[:count]


def extract(records, harmonics, state, keep, capacity):
    """records: (count, record bytes) uint8; harmonics: (count, row bytes) uint8 (row bytes may be 0).
    -> (kept ids truncated to the capacity, K, record rows, harmonics rows, state bytes)"""
    count = len(records)
    s = states_of(state, count)
    ids = np.nonzero(keep_bits(keep)[s])[0].astype(np.uint32)
    K = len(ids)
    ids = ids[:min(K, capacity)]
    return ids, K, records[ids], harmonics[ids], s[ids]


def histogram(state, count):
    return np.bincount(states_of(state, count), minlength=256).astype(np.uint32)
