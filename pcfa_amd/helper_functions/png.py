"""A minimal PNG writer for 8-bit RGB pictures: signature, IHDR, one IDAT, IEND (PNG specification, ISO/IEC 15948).

Standard library only (zlib, struct).  The bytes depend on the pixels alone -- no time stamp, no text chunk -- so two runs
write identical files.  Every row uses filter type 0 (None): the pictures written here are noise-like perturbations and
smooth colour codes whose deflate time, not size, is what a run pays for (profiles/save_png/README.md).
"""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
LEVEL = 1   # zlib level: the fastest that still compresses (profiles/save_png/README.md)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def encode_rgb8(pixels, level=LEVEL):
    """PNG file bytes of `pixels`: a uint8 array [H,W,3] (anything with .shape and .tobytes(), C order)."""
    shape = tuple(pixels.shape)
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("an RGB picture is [H,W,3] with H, W >= 1, got %s" % (shape,))
    if getattr(pixels, "dtype", None) is not None and str(pixels.dtype) != "uint8":
        raise TypeError("an 8-bit picture is uint8, got %s" % pixels.dtype)
    h, w = shape[0], shape[1]
    raw = pixels.tobytes()
    row = 3 * w
    if len(raw) != h * row:
        raise ValueError("picture data has %d bytes, expected %d" % (len(raw), h * row))
    # every scanline is preceded by its filter type; 0 = None
    filtered = bytearray(h * (row + 1))
    view = memoryview(filtered)
    for y in range(h):
        view[y * (row + 1) + 1:(y + 1) * (row + 1)] = raw[y * row:(y + 1) * row]
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)   # 8 bits, colour type 2 (RGB), deflate, adaptive filters, no interlace
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(bytes(filtered), level)) + _chunk(b"IEND", b"")


def write_rgb8(path, pixels, level=LEVEL):
    data = encode_rgb8(pixels, level)
    with open(path, "wb") as f:
        f.write(data)
    return path
