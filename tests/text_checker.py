"""Definition-level numpy restatement of the reference's semantics on general byte text (``&[u8]``), shared by
tests/test_text_cpu.py (which pins it to the oracle on 2-bit code bytes) and tests/test_gpu_text.py.

  h_fw(i) = fw_xor ^ XOR_j rotl(fw[s[i+j]], R(k-1-j));  h_rc(i) = rc_xor ^ XOR_j rotl(rc[s[i+j]], R j)
  h = h_fw + h_rc (wrapping) when the hasher is canonical, else h_fw
  window i: leftmost / rightmost argmin of h & 0xffff0000 over k-mers i .. i+w-1 (src/sliding_min.rs:104-127,
  :196-197); canonical windows take the leftmost one when 2 #{c & 2} > l over the window's l bytes, else the
  rightmost (src/canonical.rs:18-29); then the collectors: adjacent dedup with super-k-mer first-window indices
  (src/collect.rs:15-76), closed / open syncmers (src/syncmers.rs:19-48).
"""
from __future__ import annotations

import numpy as np

KEY_MASK = np.uint32(0xFFFF0000)


def _rotl(x: np.ndarray, r: int) -> np.ndarray:
    r %= 32
    if r == 0:
        return x.copy()
    return ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


def hashes(text: np.ndarray, k: int, hasher) -> np.ndarray:
    """Hash of every k-mer of ``text`` (uint8) under a TextHasher-like object (fw, rc, rot, canonical, fw_xor,
    rc_xor), straight from the definition (no rolling)."""
    s = np.asarray(text, dtype=np.uint8)
    nk = len(s) - k + 1
    if nk <= 0:
        return np.zeros(0, dtype=np.uint32)
    fw = np.array([int(v) for v in hasher.fw], dtype=np.uint32)
    rc = np.array([int(v) for v in hasher.rc], dtype=np.uint32)
    R = int(hasher.rot) % 32
    h_fw = np.full(nk, int(hasher.fw_xor) & 0xFFFFFFFF, dtype=np.uint32)
    h_rc = np.full(nk, int(hasher.rc_xor) & 0xFFFFFFFF, dtype=np.uint32)
    for j in range(k):
        c = s[j:j + nk]
        h_fw ^= _rotl(fw[c], R * (k - 1 - j))
        if hasher.canonical:
            h_rc ^= _rotl(rc[c], R * j)
    if hasher.canonical:
        return (h_fw.astype(np.uint64) + h_rc.astype(np.uint64)).astype(np.uint32)
    return h_fw


def window_positions(text: np.ndarray, k: int, w: int, hasher, canonical: bool) -> np.ndarray:
    """Absolute position of every window's minimizer."""
    s = np.asarray(text, dtype=np.uint8)
    l = k + w - 1
    nw = len(s) - l + 1
    if nw <= 0:
        return np.zeros(0, dtype=np.uint32)
    key = hashes(s, k, hasher) & KEY_MASK
    view = np.lib.stride_tricks.sliding_window_view(key, w)[:nw]
    left = np.argmin(view, axis=1)
    sel = left
    if canonical:
        right = (w - 1) - np.argmin(view[:, ::-1], axis=1)
        odd = np.concatenate([[0], np.cumsum((s >> 1) & 1, dtype=np.int64)])
        cnt = odd[l:l + nw] - odd[:nw]
        sel = np.where(2 * cnt > l, left, right)
    return (np.arange(nw, dtype=np.int64) + sel).astype(np.uint32)


def run(text, k: int, w: int, hasher, canonical: bool = False, mode: int = 0, super_kmers: bool = False):
    """The whole path: positions (minimizers) or window indices (syncmers); with ``super_kmers`` also the index of
    the first window of each minimizer's run."""
    s = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
    p = window_positions(s, k, w, hasher, canonical)
    idx = np.arange(len(p), dtype=np.uint32)
    if mode == 0:
        keep = np.ones(len(p), dtype=bool)
        keep[1:] = p[1:] != p[:-1]
        if super_kmers:
            return p[keep], idx[keep]
        return p[keep]
    if mode == 1:
        keep = (p == idx) | (p == idx + np.uint32(w - 1))
    else:
        keep = p == idx + np.uint32(w // 2)
    return idx[keep]


def text_tables_from_dna(nt) -> tuple[list, list]:
    """fw[c] = nt.fw[c & 3], rc[c] = nt.rc[c & 3]: a 4-symbol hasher on the code bytes 0..3 themselves (their c & 2
    is the packed strand vote's bit)."""
    return [int(nt.fw[c & 3]) for c in range(256)], [int(nt.rc[c & 3]) for c in range(256)]


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """2-bit codes -> packed-seq bytes (base i at bits 2(i%4) of byte i/4), with the oracle's 16 bytes of slack."""
    c = np.asarray(codes, dtype=np.uint8) & 3
    pad = np.zeros((-len(c)) % 4, dtype=np.uint8)
    q = np.concatenate([c, pad]).reshape(-1, 4)
    packed = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)
    return np.concatenate([packed, np.zeros(16, dtype=np.uint8)])


def english_like(n: int, seed: int) -> np.ndarray:
    """Skewed letters: English letter frequencies, spaces and a little punctuation."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b" etaoinshrdlcumwfgypbvkjxqz.,\n", dtype=np.uint8)
    freq = np.array([18, 12.7, 9.1, 8.2, 7.5, 7.0, 6.7, 6.3, 6.1, 6.0, 4.3, 4.0, 2.8, 2.8, 2.4, 2.4, 2.2, 2.0,
                     2.0, 1.9, 1.5, 1.0, 0.8, 0.15, 0.15, 0.1, 0.07, 1.0, 1.0, 0.8])
    return alphabet[rng.choice(len(alphabet), size=n, p=freq / freq.sum())]
