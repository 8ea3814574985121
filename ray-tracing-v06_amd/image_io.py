"""Image output on the caller's side of the path — write_renderbuffer of the reference app
(main/src/FirstApp.cpp:108-122): 8-bit conversion `uint8(v * 255.999f)` of R, G, B (alpha dropped), rows flipped
(row 0 of the framebuffer is the BOTTOM of the picture, Renderer.cu:192), then an image file.  The reference
writes JPEG q95 through stb_image_write; here PNG (lossless, zlib from the standard library) and binary PPM.
A NaN channel (NaN pixels) is written as 0: the reference's static_cast of NaN is undefined
behaviour and yields 0 on x86.
read_ppm and read_png go the other way, for texture images (Scene.set_image).
"""
import struct
import zlib

import numpy as np


def to_rgb8(framebuffer):
    """float RGBA [H][W][4], row 0 = bottom  ->  uint8 RGB [H][W][3], row 0 = top."""
    fb = np.asarray(framebuffer, dtype=np.float32)
    if fb.ndim != 3 or fb.shape[2] != 4:
        raise ValueError("framebuffer must be [H][W][4] float32")
    rgb = fb[::-1, :, :3] * np.float32(255.999)
    rgb = np.where(np.isnan(rgb), np.float32(0.0), rgb)
    return np.clip(rgb, 0.0, 255.0).astype(np.uint8)  # truncation toward zero, like static_cast<uint8_t>


def write_ppm(path, framebuffer):
    img = to_rgb8(framebuffer)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def write_png(path, framebuffer):
    img = to_rgb8(framebuffer)
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ---------------------------------------------------------------------------------------------------------------------
# Readers, for Scene.set_image (texture images): uint8 RGB [H][W][3], row 0 = top, as the file has it.
# ---------------------------------------------------------------------------------------------------------------------
def read_ppm(path):
    """A binary PPM (P6, maxval 255; `#` comments in the header) -> uint8 [H][W][3]."""
    with open(path, "rb") as f:
        data = f.read()
    pos, fields = 0, []
    while len(fields) < 4:   # magic, width, height, maxval: tokens between whitespace, comments run to the end of their line
        while pos < len(data) and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b"#"):
            if data[pos:pos + 1] == b"#":
                while pos < len(data) and data[pos:pos + 1] != b"\n":
                    pos += 1
            else:
                pos += 1
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace() and data[pos:pos + 1] != b"#":
            pos += 1
        if start == pos:
            raise ValueError(f"{path}: truncated PPM header")
        fields.append(data[start:pos])
    if fields[0] != b"P6":
        raise ValueError(f"{path}: not a binary PPM (P6)")
    try:
        w, h, maxval = int(fields[1]), int(fields[2]), int(fields[3])
    except ValueError:
        raise ValueError(f"{path}: bad PPM header") from None
    if w <= 0 or h <= 0 or maxval != 255:
        raise ValueError(f"{path}: a PPM of positive size with maxval 255 is read (got {w} x {h}, maxval {maxval})")
    pos += 1   # the single whitespace byte behind maxval
    if len(data) - pos < w * h * 3:
        raise ValueError(f"{path}: {len(data) - pos} bytes of pixels, {w * h * 3} expected")
    return np.frombuffer(data, np.uint8, w * h * 3, pos).reshape(h, w, 3).copy()


def read_png(path):
    """An 8-bit RGB or RGBA PNG without interlacing (alpha dropped) -> uint8 [H][W][3]; all five filter types."""
    return np.ascontiguousarray(_png_pixels(path)[:, :, :3])


def read_png_alpha(path):
    """The alpha channel of an 8-bit RGBA PNG (as read_png reads it) -> uint8 [H][W], row 0 = top; None for an RGB file, which has none.  What a cutout mask
    is made of: np.repeat(alpha[:, :, None], 3, axis=2) is an image whose every channel is the opacity."""
    px = _png_pixels(path)
    return np.ascontiguousarray(px[:, :, 3]) if px.shape[2] == 4 else None


def lattice_mask(width, height, bars_u, bars_v, duty):
    """A procedural fence for cutouts: uint8 [height][width][3], 255 on bars_u vertical and bars_v horizontal bars spread evenly over the image,
    0 in the holes between them; `duty` in [0, 1] = the part of each period a bar covers.  Integer arithmetic on texel centres: the same on every machine."""
    width, height, bars_u, bars_v = int(width), int(height), int(bars_u), int(bars_v)
    if width <= 0 or height <= 0 or bars_u < 0 or bars_v < 0 or not (0.0 <= float(duty) <= 1.0):
        raise ValueError("lattice_mask: a positive size, bar counts >= 0 and a duty in [0, 1]")
    def bars(n, count):   # texel i is on a bar when the phase of its centre within its period, in units of 1 / (2 n), lies below duty
        phase = ((2 * np.arange(n, dtype=np.int64) + 1) * count) % (2 * n)
        return phase < int(round(float(duty) * 2 * n)) if count else np.zeros(n, bool)
    on = bars(width, bars_u)[None, :] | bars(height, bars_v)[:, None]
    return np.ascontiguousarray(np.repeat((on * np.uint8(255))[:, :, None], 3, axis=2).astype(np.uint8))


def _png_pixels(path):
    """read_png's decoder: uint8 [H][W][3 or 4]"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, head, idat = 8, None, []
    while pos + 8 <= len(data):
        (length,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        if len(body) != length or pos + 12 + length > len(data):
            raise ValueError(f"{path}: truncated chunk {tag!r}")
        if struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: chunk {tag!r} fails its CRC")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + length
    if head is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, colour, compression, filtering, interlace = head
    if depth != 8 or colour not in (2, 6) or compression != 0 or filtering != 0 or interlace != 0 or w == 0 or h == 0:
        raise ValueError(f"{path}: 8-bit RGB / RGBA PNGs without interlacing are read (bit depth {depth}, colour type {colour}, interlace {interlace})")
    bpp = 3 if colour == 2 else 4
    stride = w * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (stride + 1):
        raise ValueError(f"{path}: {len(raw)} bytes of scanlines, {h * (stride + 1)} expected")
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(h):
        kind = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        if kind == 0:
            cur = line
        elif kind == 2:   # Up
            cur = (line + prev) & 255
        elif kind in (1, 3, 4):   # Sub, Average, Paeth: each byte needs the reconstructed byte bpp to its left
            cur = np.zeros(stride, np.int64)
            for x in range(stride):
                a = cur[x - bpp] if x >= bpp else 0
                b = prev[x]
                if kind == 1:
                    pred = a
                elif kind == 3:
                    pred = (a + b) >> 1
                else:
                    c = prev[x - bpp] if x >= bpp else 0
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + pred) & 255
        else:
            raise ValueError(f"{path}: row {y}: unknown filter type {kind}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w, bpp)


# ---------------------------------------------------------------------------------------------------------------------
# JPEG — the format the reference app writes (`stbi_write_jpg(path, w, h, 3, data, 95)`, FirstApp.cpp:120): a baseline
# (sequential, Huffman, 8-bit) JFIF encoder with the conventions of that call: the standard Annex-K quantisation tables
# scaled for the quality (q95 -> factor 10 %), no chroma subsampling above quality 90, the standard Annex-K Huffman
# tables, rows already flipped by to_rgb8.  A lossy format: pixel values match the reference writer's only up to the DCT's
# rounding, so parity tests use PNG / PPM; this exists so that a caller gets the same kind of file the reference produces.
# ---------------------------------------------------------------------------------------------------------------------
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
_Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                  + [99] * 32)
_DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
_DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
_DC_VALS = list(range(12))
_AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
_AC_LUM_VALS = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
                0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
                0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
                0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
                0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
                0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
                0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
_AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
_AC_CHR_VALS = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
                0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
                0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
                0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
                0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
                0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
                0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def _huffman_codes(bits, vals):
    """canonical code of a (BITS, HUFFVAL) table (ITU T.81 Annex C): symbol -> (code, length)"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def _dct_blocks(plane):
    """8x8 forward DCT-II (orthonormal, the JPEG definition) of every block of a [H][W] float plane whose sides are multiples of 8"""
    k = np.arange(8)
    c = np.sqrt(2.0 / 8.0) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16.0)
    c[0, :] = np.sqrt(1.0 / 8.0)
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)           # [by][bx][8][8]
    return np.einsum("ij,yxjk,lk->yxil", c, b, c)


def write_jpg(path, framebuffer, quality=95):
    """Baseline JPEG of the framebuffer with stb_image_write's conventions for `stbi_write_jpg(..., quality)` (FirstApp.cpp:120)."""
    rgb = to_rgb8(framebuffer).astype(np.float64)
    h, w, _ = rgb.shape
    quality = min(100, max(1, int(quality)))
    scale = 5000 // quality if quality < 50 else 200 - quality * 2
    qt = [np.clip((t * scale + 50) // 100, 1, 255).astype(np.int64) for t in (_Q_LUM, _Q_CHR)]
    # JFIF colour transform, level shift, edge replication up to a multiple of 8 (no subsampling: stb subsamples only for quality <= 90)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    planes = [0.29900 * r + 0.58700 * g + 0.11400 * b - 128.0, -0.16874 * r - 0.33126 * g + 0.50000 * b, 0.50000 * r - 0.41869 * g - 0.08131 * b]
    ph, pw = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    coefs = []
    for ci, pl in enumerate(planes):
        pl = np.pad(pl, ((0, ph - h), (0, pw - w)), mode="edge")
        d = _dct_blocks(pl).reshape(ph // 8, pw // 8, 64) / qt[0 if ci == 0 else 1][None, None, :]
        q = np.where(d < 0, np.ceil(d - 0.5), np.floor(d + 0.5)).astype(np.int64)     # round half away from zero, as stb does
        coefs.append(q[..., _ZIGZAG])
    dc_tab = [_huffman_codes(_DC_LUM_BITS, _DC_VALS), _huffman_codes(_DC_CHR_BITS, _DC_VALS)]
    ac_tab = [_huffman_codes(_AC_LUM_BITS, _AC_LUM_VALS), _huffman_codes(_AC_CHR_BITS, _AC_CHR_VALS)]

    acc, nbits, out = 0, 0, bytearray()

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length
        while nbits >= 8:
            byte = (acc >> (nbits - 8)) & 0xFF
            out.append(byte)
            if byte == 0xFF:
                out.append(0)          # byte stuffing
            nbits -= 8
        acc &= (1 << nbits) - 1

    def magnitude(v):                  # (category, extra bits) of a coefficient (T.81 F.1.2.1)
        a = -v if v < 0 else v
        cat = a.bit_length()
        return cat, (v if v >= 0 else v + (1 << cat) - 1)

    prev_dc = [0, 0, 0]
    for by in range(ph // 8):
        for bx in range(pw // 8):
            for ci in range(3):
                blk = coefs[ci][by, bx]
                t = 0 if ci == 0 else 1
                diff = int(blk[0]) - prev_dc[ci]
                prev_dc[ci] = int(blk[0])
                cat, extra = magnitude(diff)
                put(*dc_tab[t][cat])
                if cat:
                    put(extra, cat)
                nz = np.nonzero(blk[1:])[0]
                pos = 0
                for k in nz:
                    run = int(k) - pos
                    while run >= 16:
                        put(*ac_tab[t][0xF0])      # ZRL: sixteen zeros
                        run -= 16
                    cat, extra = magnitude(int(blk[1 + k]))
                    put(*ac_tab[t][(run << 4) | cat])
                    put(extra, cat)
                    pos = int(k) + 1
                if pos < 63:
                    put(*ac_tab[t][0x00])          # EOB
    if nbits:
        put((1 << (8 - nbits)) - 1, 8 - nbits)     # pad the last byte with ones

    def segment(marker, payload):
        return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload

    def dht(cls_id, bits, vals):
        return bytes([cls_id]) + bytes(bits) + bytes(vals)

    head = b"\xff\xd8" + segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    head += segment(0xDB, b"\x00" + bytes(qt[0][_ZIGZAG].astype(np.uint8)) + b"\x01" + bytes(qt[1][_ZIGZAG].astype(np.uint8)))
    head += segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    head += segment(0xC4, dht(0x00, _DC_LUM_BITS, _DC_VALS) + dht(0x10, _AC_LUM_BITS, _AC_LUM_VALS)
                    + dht(0x01, _DC_CHR_BITS, _DC_VALS) + dht(0x11, _AC_CHR_BITS, _AC_CHR_VALS))
    head += segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    with open(path, "wb") as f:
        f.write(head + bytes(out) + b"\xff\xd9")


# ---- Radiance RGBE (.hdr) pictures and a procedural sky: environment maps ----
# A pixel is three 8-bit mantissas and one shared exponent: channel = (mantissa + 0.5) * 2^(e - 136), all zero bytes = black (Radiance's color.c).  The largest
# channel's mantissa is >= 128, so a channel is off by at most 2^-8 of the LARGEST channel of its pixel after a round trip.
def _rgbe_encode(rgb):
    rgb = np.asarray(rgb, dtype=np.float64)
    v = rgb.max(axis=-1)
    m, e = np.frexp(v)
    ok = v >= 1e-32
    scale = np.where(ok, m * 256.0 / np.where(ok, v, 1.0), 0.0)
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.clip(np.floor(rgb * scale[..., None]), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    out[~ok] = 0
    return out


def _rgbe_decode(rgbe):
    e = rgbe[..., 3].astype(np.int32)
    f = np.ldexp(1.0, e - 136)
    out = (rgbe[..., :3].astype(np.float64) + 0.5) * f[..., None]
    out[e == 0] = 0.0
    return out.astype(np.float32)


def write_hdr(path, image):
    """A Radiance RGBE picture of image (H, W, 3) float, finite and >= 0, row 0 at the top: `-Y H +X W`, flat scanlines."""
    img = np.asarray(image, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError("write_hdr: the image must have shape (H, W, 3)")
    if not np.isfinite(img).all() or (img < 0).any():
        raise ValueError("write_hdr: values must be finite and >= 0")
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode("ascii") + _rgbe_encode(img).tobytes())


def read_hdr(path):
    """A Radiance RGBE picture as (H, W, 3) float32, row 0 at the top.  Flat and new-style run-length encoded scanlines, orientation `-Y H +X W` only;
    anything else raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    if not data.startswith(b"#?"):
        raise ValueError("read_hdr: not a Radiance picture (no #? signature)")
    pos, fmt = 0, None
    while True:
        end = data.find(b"\n", pos)
        if end < 0:
            raise ValueError("read_hdr: the header does not end")
        line = data[pos:end]
        pos = end + 1
        if not line:
            break
        if line.startswith(b"FORMAT="):
            fmt = line[7:].strip()
    if fmt != b"32-bit_rle_rgbe":
        raise ValueError(f"read_hdr: FORMAT must be 32-bit_rle_rgbe, not {fmt!r}")
    end = data.find(b"\n", pos)
    parts = data[pos:end].split() if end >= 0 else []
    if len(parts) != 4 or parts[0] != b"-Y" or parts[2] != b"+X" or not parts[1].isdigit() or not parts[3].isdigit():
        raise ValueError("read_hdr: the resolution line must read -Y H +X W")
    h, w = int(parts[1]), int(parts[3])
    if h == 0 or w == 0:
        raise ValueError("read_hdr: empty picture")
    pos = end + 1
    out = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        if 8 <= w <= 0x7fff and data[pos:pos + 2] == b"\x02\x02" and pos + 4 <= len(data) and data[pos + 2] < 128:   # a new-style run-length encoded scanline
            if (data[pos + 2] << 8 | data[pos + 3]) != w:
                raise ValueError(f"read_hdr: scanline {y}: its length does not match the width")
            pos += 4
            for c in range(4):   # the four bytes of every pixel are coded apart
                x = 0
                while x < w:
                    if pos >= len(data):
                        raise ValueError(f"read_hdr: scanline {y}: the data ends early")
                    count = data[pos]
                    pos += 1
                    if count > 128:   # a run: count - 128 copies of one byte
                        count -= 128
                        if x + count > w or pos >= len(data):
                            raise ValueError(f"read_hdr: scanline {y}: a run passes the end of the line")
                        out[y, x:x + count, c] = data[pos]
                        pos += 1
                    else:             # count bytes as they are
                        if count == 0 or x + count > w or pos + count > len(data):
                            raise ValueError(f"read_hdr: scanline {y}: a bad literal count")
                        out[y, x:x + count, c] = np.frombuffer(data, np.uint8, count, pos)
                        pos += count
                    x += count
        else:   # flat: four bytes per pixel
            if pos + 4 * w > len(data):
                raise ValueError(f"read_hdr: scanline {y}: the data ends early")
            row = np.frombuffer(data, np.uint8, 4 * w, pos).reshape(w, 4)
            if ((row[:, 0] == 1) & (row[:, 1] == 1) & (row[:, 2] == 1)).any():
                raise ValueError(f"read_hdr: scanline {y}: old-style run-length encoding is not read")
            out[y] = row
            pos += 4 * w
    return _rgbe_decode(out)


def sky_environment(width, height, sun_dir=(0.4, 0.6, -0.7), sun_radiance=(60.0, 54.0, 45.0), sun_radius_deg=4.0, zenith=(0.15, 0.3, 0.8), horizon=(0.8, 0.85, 0.9),
                    ground=(0.25, 0.22, 0.2)):
    """A procedural HDR sky as an environment map (H, W, 3) float32, row 0 at the top, in the layout the lookup reads with u0 = 0: a gradient from
    the horizon to the zenith, a flat ground below the horizon, a sun disc of sun_radiance within sun_radius_deg of sun_dir and a glow around it."""
    u = (np.arange(width, dtype=np.float64) + 0.5) / width
    theta = np.pi * (1.0 - (np.arange(height, dtype=np.float64) + 0.5) / height)   # of the lookup: acos(-n.y); row 0 looks up
    a = 2.0 * np.pi * u - np.pi                                                   # atan2(-n.z, n.x)
    ny = -np.cos(theta)[:, None] * np.ones((1, width))
    nx = np.sin(theta)[:, None] * np.cos(a)[None, :]
    nz = -np.sin(theta)[:, None] * np.sin(a)[None, :]
    s = np.asarray(sun_dir, dtype=np.float64)
    s = s / np.sqrt((s * s).sum())
    up = np.clip(ny, 0.0, 1.0)[..., None]
    sky = np.asarray(horizon, np.float64) * (1.0 - up) + np.asarray(zenith, np.float64) * up
    img = np.where((ny >= 0.0)[..., None], sky, np.asarray(ground, np.float64))
    cos_sun = nx * s[0] + ny * s[1] + nz * s[2]
    sun = np.asarray(sun_radiance, np.float64)
    glow = np.clip(cos_sun, 0.0, 1.0) ** 64
    img = img + (ny >= 0.0)[..., None] * glow[..., None] * sun * 0.02
    img = np.where((cos_sun >= np.cos(np.radians(sun_radius_deg)))[..., None], sun, img)
    return np.ascontiguousarray(img, dtype=np.float32)


def height_to_normal_map(height, scale=1.0, wrap="repeat"):
    """A grey height field (H, W), row 0 at the top, as a tangent-space normal map (H, W, 3) uint8 for Scene.set_normal_map (OpenGL convention:
    red = +u, the columns' direction; green = +v, towards row 0; blue = along the surface normal).  Central differences per texel, the neighbours wrapped
    ("repeat") or clamped ("clamp") as the image's wrap mode will have them: n = normalize(-scale dh/du, -scale dh/dv, 1), byte = 128 + round(127 n), which
    the rule decodes as (byte - 128) / 127.  A constant field gives the flat map (128, 128, 255)."""
    h = np.asarray(height, dtype=np.float64)
    if h.ndim != 2 or h.size == 0:
        raise ValueError("height_to_normal_map: the height field must have shape (H, W)")
    if wrap not in ("repeat", "clamp"):
        raise ValueError("height_to_normal_map: wrap is \"repeat\" or \"clamp\"")
    if wrap == "repeat":
        right, left, up, down = np.roll(h, -1, axis=1), np.roll(h, 1, axis=1), np.roll(h, 1, axis=0), np.roll(h, -1, axis=0)
    else:
        p = np.pad(h, 1, mode="edge")
        right, left, up, down = p[1:-1, 2:], p[1:-1, :-2], p[:-2, 1:-1], p[2:, 1:-1]
    dhdu, dhdv = (right - left) * 0.5, (up - down) * 0.5   # v grows towards row 0
    n = np.stack([-float(scale) * dhdu, -float(scale) * dhdv, np.ones_like(h)], axis=-1)
    n = n / np.sqrt((n * n).sum(axis=-1, keepdims=True))
    return np.ascontiguousarray(np.clip(128.0 + np.rint(127.0 * n), 0.0, 255.0).astype(np.uint8))
