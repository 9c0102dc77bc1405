"""A small PNG codec for the evaluation / prediction pictures: 8-bit RGBA, non-interlaced, ``zlib`` and ``struct`` from the
standard library and nothing else (matplotlib and PIL are no dependencies).

``write_rgba`` writes one IHDR, one IDAT and one IEND chunk; every scanline carries the same filter type.  The bytes are a
pure function of the array (no time stamp, no text chunk).  ``read_rgba`` reads any 8-bit RGBA, non-interlaced file, all
five filter types, so it reads whatever ``write_rgba`` emits with any setting, and such files of other writers.

``FILTER`` and ``LEVEL`` are the defaults chosen from the table of ``tools/bench_png.py``."""
from __future__ import annotations

import struct
import zlib
from pathlib import Path
from typing import Union

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTER_NONE, FILTER_SUB, FILTER_UP, FILTER_AVERAGE, FILTER_PAETH = range(5)
# measured per 256x512 picture: on a scan with lines over it, speckle leaves a row or a neighbour no
# better a predictor than nothing -- no filter gives the smallest file at every level (177 KB at level 1 against 188 / 193
# with sub / up) and the shortest encode (3.3 ms); level 6 costs 7x the time for 10 % fewer bytes.  Class maps take 0.5 ms
# and 3.4-3.7 KB with every filter at level 1.
FILTER = FILTER_NONE
LEVEL = 1


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_rgba(arr: np.ndarray, filter_type: int = None, level: int = None) -> bytes:
    """(H, W, 4) uint8 -> the bytes of the PNG file.  ``filter_type`` 0 (none), 1 (sub) or 2 (up)."""
    a = np.asarray(arr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_rgba takes a uint8 (H, W, 4) array, not {a.dtype} {a.shape}")
    f = FILTER if filter_type is None else int(filter_type)
    lv = LEVEL if level is None else int(level)
    H, W, _ = a.shape
    a = np.ascontiguousarray(a)
    if f == FILTER_NONE:
        body = a
    elif f == FILTER_SUB:
        body = a.copy()
        body[:, 1:] -= a[:, :-1]                 # uint8 arithmetic wraps modulo 256, which is the filter's definition
    elif f == FILTER_UP:
        body = a.copy()
        body[1:] -= a[:-1]
    else:
        raise ValueError(f"write_rgba emits filter types 0, 1 and 2, not {f}")
    lines = np.empty((H, 1 + 4 * W), np.uint8)
    lines[:, 0] = f
    lines[:, 1:] = body.reshape(H, 4 * W)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(lines.tobytes(), lv)) + _chunk(b"IEND", b"")


def write_rgba(path: Union[str, Path], arr: np.ndarray, filter_type: int = None, level: int = None) -> None:
    data = encode_rgba(arr, filter_type, level)
    with open(path, "wb") as fh:
        fh.write(data)


def decode_rgba(data: bytes) -> np.ndarray:
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file")
    pos, idat, shape = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"PNG chunk {kind!r}: CRC mismatch")
        pos += 12 + n
        if kind == b"IHDR":
            W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", body)
            if (depth, colour, comp, filt, interlace) != (8, 6, 0, 0, 0):
                raise ValueError("read_rgba reads 8-bit RGBA, non-interlaced PNG files only")
            shape = (H, W)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if shape is None or not idat:
        raise ValueError("PNG file without IHDR or IDAT")
    H, W = shape
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != H * (1 + 4 * W):
        raise ValueError("PNG data of the wrong length")
    lines = raw.reshape(H, 1 + 4 * W)
    out = np.zeros((H, W, 4), np.uint8)
    prev = np.zeros((W, 4), np.uint8)
    for r in range(H):
        f, x = int(lines[r, 0]), lines[r, 1:].reshape(W, 4)
        if f == FILTER_NONE:
            cur = x.copy()
        elif f == FILTER_SUB:
            cur = np.cumsum(x, axis=0, dtype=np.uint8)                       # wraps modulo 256
        elif f == FILTER_UP:
            cur = x + prev
        elif f in (FILTER_AVERAGE, FILTER_PAETH):
            cur = np.zeros((W, 4), np.int64)
            up = prev.astype(np.int64)
            xi = x.astype(np.int64)
            left, upleft = np.zeros(4, np.int64), np.zeros(4, np.int64)
            for c in range(W):
                if f == FILTER_AVERAGE:
                    pred = (left + up[c]) >> 1
                else:
                    p = left + up[c] - upleft
                    pa, pb, pc = np.abs(p - left), np.abs(p - up[c]), np.abs(p - upleft)
                    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up[c], upleft))
                cur[c] = (xi[c] + pred) & 255
                left, upleft = cur[c], up[c]
            cur = cur.astype(np.uint8)
        else:
            raise ValueError(f"PNG filter type {f}")
        out[r] = cur
        prev = cur
    return out


def read_rgba(path: Union[str, Path]) -> np.ndarray:
    """The (H, W, 4) uint8 pixels of an 8-bit RGBA, non-interlaced PNG file."""
    with open(path, "rb") as fh:
        return decode_rgba(fh.read())
