"""Writer of image sequences the way the fork's encoder lays them out (test tool): coded HEVC-intra pictures
([u32 BE len][NAL] strings) become the samples of one 'moov' track -
ftyp{.. 'hevc' ..} / moov{mvhd, trak{tkhd, mdia{mdhd, hdlr, minf{vmhd, stbl{stsd{hvc1{hvcC, ccst}}, stts, stss, stsc, stsz,
stco}}}}} / mdat  (libheif/context.cc:3074-3081, box.cc:1616-1690 of the reference) - and a Python restatement of what the
fork hands its decoder for one sample (codecs/hevc.cc:196-224, file.cc:1154-1244)."""
import struct

import heifwriter

PARAM_TYPES = (32, 33, 34)  # VPS, SPS, PPS


def _box(t, payload):
    return struct.pack(">I4s", 8 + len(payload), t) + payload


def _full(t, version, flags, payload):
    return _box(t, bytes([version]) + flags.to_bytes(3, "big") + payload)


def _nal_type(n):
    return (n[0] >> 1) & 0x3F


def _hvcc(arrays, chroma_format, bit_depth):
    """arrays: list of (nal_type, [units])"""
    body = bytes([1, 1]) + b"\x60\x00\x00\x00" + b"\x90\x00\x00\x00\x00\x00" + bytes([183])
    body += b"\xf0\x00" + b"\xfc" + bytes([0xFC | chroma_format, 0xF8 | (bit_depth - 8), 0xF8 | (bit_depth - 8)])
    body += b"\x00\x00" + bytes([0x0F])
    body += bytes([len(arrays)])
    for t, units in arrays:
        body += bytes([0x80 | t]) + struct.pack(">H", len(units))
        for n in units:
            body += struct.pack(">H", len(n)) + n
    return _box(b"hvcC", body)


def _hvc1(width, height, n_frames, children, compressorname=b"HEVC Coding"):
    # the fork's sample entry (box.cc:1580-1603): compressorname written as a NUL-terminated string padded to 32 bytes
    body = bytes(6) + struct.pack(">H", 1) + struct.pack(">HH", 0, 0) + bytes(12)
    body += struct.pack(">HH", width, height) + struct.pack(">III", 0x00480000, 0x00480000, 0) + struct.pack(">H", n_frames & 0xFFFF)
    name = compressorname + b"\x00"
    body += name + bytes(max(0, 32 - len(name)))
    body += struct.pack(">Hh", 0x18, -1)
    return _box(b"hvc1", body + children)


def write_movie(pictures, size, chroma_format=1, bit_depth=8, constant_size=False, params_in="hvcc", hvcc_units=None,
                duration=3000, timescale=1000, version=0, meta=None, brands=(b"msf1", b"iso8", b"hevc"), stsc_entries=None,
                stsz_entries=None, samples_per_chunk=None, chunk_offset_delta=0, omit=(), compressorname=b"HEVC Coding", major=None):
    """pictures: [len][NAL] strings, each VPS/SPS/PPS + slice(s); size: (w, h) written into tkhd (16.16) and hvc1.
    params_in: "hvcc" - every frame's parameter sets go into the hvcC arrays (unit k of each array = frame k+1's), the samples
    hold the slices; "sample" - the hvcC holds the first frame's parameter sets, every sample its own ones and its slices.
    hvcc_units: keep only the first n units of every hvcC array (frames past n reuse the last one).
    constant_size: one 'stsz' size for all samples (they must be equally long).
    meta: optional bytes of a 'meta' box (e.g. from heifwriter) written beside the 'moov'.
    brands: the ftyp's compatible brands; major: its major brand (default: the first compatible one).
    stsc_entries / stsz_entries / samples_per_chunk / chunk_offset_delta / omit: broken tables for refusal tests."""
    n = len(pictures)
    frames = [heifwriter.split_nals(p) for p in pictures]
    params = [[u for u in f if _nal_type(u) in PARAM_TYPES] for f in frames]
    arrays = []
    for t in PARAM_TYPES:
        if params_in == "hvcc":
            units = [next(u for u in ps if _nal_type(u) == t) for ps in params]
        else:
            units = [next(u for u in params[0] if _nal_type(u) == t)]
        if hvcc_units is not None:
            units = units[:hvcc_units]
        arrays.append((t, units))
    samples = []
    for f in frames:
        keep = f if params_in == "sample" else [u for u in f if _nal_type(u) not in PARAM_TYPES]
        samples.append(b"".join(struct.pack(">I", len(u)) + u for u in keep))
    w, h = size

    def build(chunk_offset):
        if version == 1:
            mvhd = _full(b"mvhd", 1, 0, struct.pack(">QQIQ", 0, 0, timescale, duration) + struct.pack(">IHH", 0x00010000, 0x0100, 0)
                         + bytes(8) + bytes(36) + bytes(24) + struct.pack(">I", 2))
            tkhd_t = struct.pack(">QQIIQ", 0, 0, 1, 0, duration)
        else:
            mvhd = _full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, timescale, duration & 0xFFFFFFFF) + struct.pack(">IHH", 0x00010000, 0x0100, 0)
                         + bytes(8) + bytes(36) + bytes(24) + struct.pack(">I", 2))
            tkhd_t = struct.pack(">IIIII", 0, 0, 1, 0, duration & 0xFFFFFFFF)
        tkhd = _full(b"tkhd", version, 1, tkhd_t + bytes(8) + struct.pack(">HHHH", 0, 0, 0, 0) + bytes(36) + struct.pack(">II", w << 16, h << 16))
        mdhd = _full(b"mdhd", 0, 0, struct.pack(">IIII", 0, 0, timescale, duration & 0xFFFFFFFF) + struct.pack(">HH", 0x55C4, 0))
        hdlr = _full(b"hdlr", 0, 0, bytes(4) + b"pict" + bytes(12) + b"\x00")
        vmhd = _full(b"vmhd", 0, 1, bytes(8))
        ccst = _full(b"ccst", 0, 0, bytes([(1 << 7) | (1 << 6) | (15 << 2), 0, 0, 0]))
        hvcc = b"" if b"hvcC" in omit else _hvcc(arrays, chroma_format, bit_depth)
        hvc1 = _hvc1(w, h, n, hvcc + ccst, compressorname)
        stsd = _full(b"stsd", 0, 0, struct.pack(">I", 1) + hvc1)
        stts = _full(b"stts", 0, 0, struct.pack(">III", 1, n, (duration // max(n, 1)) & 0xFFFFFFFF))
        stss = _full(b"stss", 0, 0, struct.pack(">I", n) + b"".join(struct.pack(">I", k + 1) for k in range(n)))
        entries = stsc_entries if stsc_entries is not None else [(1, n if samples_per_chunk is None else samples_per_chunk, 1)]
        stsc = _full(b"stsc", 0, 0, struct.pack(">I", len(entries)) + b"".join(struct.pack(">III", *e) for e in entries))
        if constant_size:
            assert len(set(len(s) for s in samples)) == 1, "constant 'stsz' size needs equally long samples"
            stsz = _full(b"stsz", 0, 0, struct.pack(">II", len(samples[0]), n))
        else:
            sizes = [len(s) for s in samples] if stsz_entries is None else stsz_entries
            stsz = _full(b"stsz", 0, 0, struct.pack(">II", 0, len(sizes)) + b"".join(struct.pack(">I", s) for s in sizes))
        stco = _full(b"stco", 0, 0, struct.pack(">II", 1, chunk_offset))
        tables = [(b"stsd", stsd), (b"stts", stts), (b"stss", stss), (b"stsc", stsc), (b"stsz", stsz), (b"stco", stco)]
        stbl = _box(b"stbl", b"".join(b for t, b in tables if t not in omit))
        minf = _box(b"minf", vmhd + stbl)
        mdia = _box(b"mdia", mdhd + hdlr + minf)
        trak = _box(b"trak", tkhd + mdia)
        moov = _box(b"moov", mvhd + trak)
        ftyp = _box(b"ftyp", (major or brands[0]) + struct.pack(">I", 0) + b"".join(brands))
        return ftyp + (meta or b"") + moov

    head = build(0)
    mdat_payload = b"".join(samples)
    offset = len(head) + 8
    head = build(offset + chunk_offset_delta)
    assert len(head) + 8 == offset
    return head + _box(b"mdat", mdat_payload)


# ---- the fork's reading of such a file, restated ------------------------------------------------------------------------

def top_box(buf, t):
    """the whole top-level box of type t (header included)"""
    return next(bytes(buf[b0 - 8:b1]) for bt, b0, b1 in _boxes(buf, 0, len(buf)) if bt == t)


def _boxes(buf, pos, end):
    while pos + 8 <= end:
        size, t = struct.unpack_from(">I4s", buf, pos)
        hdr = 8
        if size == 1:
            size = struct.unpack_from(">Q", buf, pos + 8)[0]
            hdr = 16
        elif size == 0:
            size = end - pos
        yield t, pos + hdr, pos + size
        pos += size


def _child(buf, pos, end, t):
    for bt, b0, b1 in _boxes(buf, pos, end):
        if bt == t:
            return b0, b1
    raise KeyError(t)


def fork_movie_info(buf):
    """frame_count, duration, (width, height) of the track, and the pieces the sample bytes are made of"""
    moov = _child(buf, 0, len(buf), b"moov")
    mvhd = _child(buf, *moov, b"mvhd")
    ver = buf[mvhd[0]]
    duration = struct.unpack_from(">Q", buf, mvhd[0] + 4 + 20)[0] if ver == 1 else struct.unpack_from(">I", buf, mvhd[0] + 4 + 12)[0]
    trak = _child(buf, *moov, b"trak")
    tkhd = _child(buf, *trak, b"tkhd")
    tv = buf[tkhd[0]]
    o = tkhd[0] + 4 + (32 if tv == 1 else 20) + 8 + 8 + 36
    tw, th = struct.unpack_from(">II", buf, o)
    stbl = _child(buf, *_child(buf, *_child(buf, *trak, b"mdia"), b"minf"), b"stbl")
    stsd = _child(buf, *stbl, b"stsd")
    hvc1 = _child(buf, stsd[0] + 8, stsd[1], b"hvc1")
    p = hvc1[0] + 42
    name_len = buf.index(b"\x00", p) - p
    assert name_len <= 31
    p += 32 + 4
    hvcc = _child(buf, p, hvc1[1], b"hvcC")
    q = hvcc[0] + 23
    arrays = []
    for _ in range(buf[q - 1]):  # (numOfArrays at byte 22)
        nn = struct.unpack_from(">H", buf, q + 1)[0]
        q += 3
        units = []
        for _ in range(nn):
            ln = struct.unpack_from(">H", buf, q)[0]
            if ln:
                units.append(bytes(buf[q + 2:q + 2 + ln]))
            q += 2 + ln
        arrays.append(units)
    stsz = _child(buf, *stbl, b"stsz")
    const, cnt = struct.unpack_from(">II", buf, stsz[0] + 4)
    sizes = [] if const else list(struct.unpack_from(">%dI" % cnt, buf, stsz[0] + 12))
    stsc = _child(buf, *stbl, b"stsc")
    spc = struct.unpack_from(">I", buf, stsc[0] + 4 + 4 + 4)[0]
    stco = _child(buf, *stbl, b"stco")
    base = struct.unpack_from(">I", buf, stco[0] + 8)[0]
    return dict(frame_count=spc, duration=duration, width=tw >> 16, height=th >> 16, arrays=arrays, const=const, sizes=sizes, base=base)


def fork_sample_bytes(buf, item_id, info=None):
    """Box_hvcC::get_header(ID-1) + get_image_data_for_moov(ID): what the fork pushes to its decoder for sample ID"""
    info = info or fork_movie_info(buf)
    out = b""
    for units in info["arrays"]:
        u = units[item_id - 1] if item_id - 1 < len(units) else units[-1]
        out += struct.pack(">I", len(u)) + u
    k = item_id - 1
    size = info["const"] or info["sizes"][k]
    off = info["base"] + (info["const"] * k if info["const"] else sum(info["sizes"][:k]))
    return out + bytes(buf[off:off + size])
