"""A minimal PNG writer for 8-bit RGB pictures: signature, IHDR, one IDAT, IEND (PNG specification, ISO/IEC 15948) -- and
the host half of a PNG reader for the dataset files: the container (chunks, CRCs, inflate) with every property checked,
which hands the still FILTERED scanlines on; undoing the filters is per-pixel work and belongs to the device
(ops.png_unfilter), with `unfilter_reference` as its plain-loop statement for the CPU path and the tests.

Standard library only (zlib, struct) plus numpy for one strided maximum.  The bytes depend on the pixels alone -- no time stamp, no text chunk -- so two runs
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


# ---------------------------------------------------------------------------------------------------------- read side
# (colour type, bit depth) -> (bytes per complete pixel, what the samples are): the formats of Sintel, KITTI-15 and the
# reference's reader; everything else is refused
FORMATS = {(2, 8): (3, "rgb8"), (0, 8): (1, "grey8"), (6, 8): (4, "rgba8"), (2, 16): (6, "rgb16")}


def decode_header_and_scanlines(data):
    """(width, height, bit depth, colour type, scanlines) of the PNG file bytes `data`.  `scanlines` are the inflated,
    still filtered rows: H times one filter-type byte followed by row_bytes = W * bytes-per-pixel bytes, all IDAT chunks
    concatenated before inflating.  A file is outside input, so everything is checked and each failure is a ValueError
    naming the property: signature, IHDR first, every chunk's CRC, compression and filter method 0, no interlace, a
    served format (FORMATS), the inflated length, every filter type <= 4."""
    import numpy as np
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ValueError("PNG signature: the file does not start with the eight signature bytes")
    pos, first, ihdr, idat, ended = 8, True, None, [], False
    while pos < len(data):
        if pos + 8 > len(data):
            raise ValueError("PNG chunk header: truncated at byte %d" % pos)
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + length > len(data):
            raise ValueError("PNG chunk %r: truncated (%d bytes declared at byte %d)" % (kind, length, pos))
        body = data[pos + 8:pos + 8 + length]
        crc, = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        if crc != (zlib.crc32(kind + body) & 0xffffffff):
            raise ValueError("PNG chunk %r: CRC mismatch" % kind)
        if first and kind != b"IHDR":
            raise ValueError("PNG IHDR: the first chunk is %r" % kind)
        first = False
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise ValueError("PNG IHDR: repeated or not 13 bytes long")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        pos += 12 + length
    if ihdr is None:
        raise ValueError("PNG IHDR: missing")
    if not ended:
        raise ValueError("PNG IEND: missing (truncated file)")
    w, h, depth, ctype, compression, filter_method, interlace = ihdr
    if w < 1 or h < 1:
        raise ValueError("PNG size: %d x %d" % (w, h))
    if compression != 0:
        raise ValueError("PNG compression method: %d (only 0, deflate, exists)" % compression)
    if filter_method != 0:
        raise ValueError("PNG filter method: %d (only 0, the five adaptive filters, exists)" % filter_method)
    if interlace != 0:
        raise ValueError("PNG interlace method: %d (Adam7 files are not served)" % interlace)
    if (ctype, depth) not in FORMATS:
        raise ValueError("PNG format: colour type %d at %d bits is not served (8-bit RGB / grey / RGBA and 16-bit RGB are; "
                         "palette images and other depths are not)" % (ctype, depth))
    row_bytes = w * FORMATS[(ctype, depth)][0]
    inflater = zlib.decompressobj()
    try:
        scanlines = inflater.decompress(b"".join(idat), h * (1 + row_bytes) + 1)   # (never inflates a bomb past one byte extra)
    except zlib.error as e:
        raise ValueError("PNG IDAT: inflate failed (%s)" % e)
    if len(scanlines) != h * (1 + row_bytes) or not inflater.eof:
        raise ValueError("PNG inflated length: %s%d bytes, %d x (1 + %d) = %d expected"
                         % ("" if inflater.eof else "stream not finished after ", len(scanlines), h, row_bytes,
                            h * (1 + row_bytes)))
    worst = int(np.frombuffer(scanlines, np.uint8)[::1 + row_bytes].max())
    if worst > 4:
        raise ValueError("PNG filter type: a scanline starts with %d (0..4 exist)" % worst)
    return w, h, depth, ctype, scanlines


def unfilter_reference(scanlines, H, row_bytes, bpp):
    """The H * row_bytes reconstructed bytes of H filtered scanlines (1 filter-type byte + row_bytes each): the PNG
    specification's five reconstruction rules as a plain loop over bytes, bpp = bytes per complete pixel.  SLOW -- about a
    microsecond per byte, seconds for one dataset frame -- and meant to be: it is the statement the device kernel
    (ops.png_unfilter) is tested against, and the path of a CPU run."""
    if len(scanlines) != H * (1 + row_bytes):
        raise ValueError("%d scanline bytes, %d x (1 + %d) expected" % (len(scanlines), H, row_bytes))
    out = bytearray(H * row_bytes)
    zero = bytes(row_bytes)
    for y in range(H):
        ft = scanlines[y * (1 + row_bytes)]
        line = scanlines[y * (1 + row_bytes) + 1:(y + 1) * (1 + row_bytes)]
        prior = out[(y - 1) * row_bytes:y * row_bytes] if y else zero
        cur = bytearray(row_bytes)
        for i in range(row_bytes):
            a = cur[i - bpp] if i >= bpp else 0          # left
            b = prior[i]                                 # up
            c = prior[i - bpp] if i >= bpp else 0        # upper left
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) >> 1
            elif ft == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            else:
                raise ValueError("filter type %d in row %d" % (ft, y))
            cur[i] = (line[i] + pred) & 255
        out[y * row_bytes:(y + 1) * row_bytes] = cur
    return bytes(out)
