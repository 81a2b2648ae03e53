"""gainwriter.py - TEST TOOL: HEIF files with a 'tmap' item (ISO 21496-1 gain map) over overlaywriter.Writer: the item, its payload
as include/heif_mi355x.h states it, its two 'dimg' references (base image, gain-map image), its 'colr' and 'clli' - and auxiliary
images with a URN of the caller's choice (a vendor gain map among the 'auxl' items).

    w = Writer()
    base = w.hvc1(picture, (64, 64))
    gmap = w.hvc1(map_picture, (32, 32), chroma_format=0, hidden=True)
    t = w.tmap(base, gmap, tmap_payload(PARAMS), (64, 64), colr=(9, 16, 0, 1), clli=(1000, 400))
    data = w.finish(primary=base)

A fraction is a (numerator, denominator) pair of integers; a channel is a dict of the five fractions min, max, gamma, base_offset,
alternate_offset."""
import struct

import overlaywriter
from hdrwriter import clli_box
from heifwriter import _colr, _full

CHANNEL_FIELDS = (("min", ">i"), ("max", ">i"), ("gamma", ">I"), ("base_offset", ">i"), ("alternate_offset", ">i"))


def channel(min=(0, 1), max=(2, 1), gamma=(1, 1), base_offset=(1, 64), alternate_offset=(1, 64)):
    return dict(min=min, max=max, gamma=gamma, base_offset=base_offset, alternate_offset=alternate_offset)


def tmap_payload(channels, base_headroom=(0, 1), alternate_headroom=(2, 1), version=0, minimum_version=0, writer_version=0, use_base=False,
                 multichannel=None, extra_flags=0):
    """channels: one channel (it stands for all three) or three; multichannel: the flag as written (default: what the count says)"""
    channels = list(channels)
    if multichannel is None:
        multichannel = len(channels) == 3
    out = struct.pack(">BHHB", version, minimum_version, writer_version, (0x80 if multichannel else 0) | (0x40 if use_base else 0) | extra_flags)
    out += struct.pack(">II", *base_headroom) + struct.pack(">II", *alternate_headroom)
    for ch in channels:
        for name, fmt in CHANNEL_FIELDS:
            out += struct.pack(fmt, ch[name][0]) + struct.pack(">I", ch[name][1])
    return out


def as_doubles(channels, base_headroom=(0, 1), alternate_headroom=(2, 1)):
    """what hm_file_gain_map_info hands out for such a payload: (Hb, Ha, {field: [three doubles]})"""
    channels = list(channels)
    three = channels if len(channels) == 3 else channels * 3
    return (base_headroom[0] / base_headroom[1], alternate_headroom[0] / alternate_headroom[1],
            {name: [ch[name][0] / ch[name][1] for ch in three] for name, _ in CHANNEL_FIELDS})


class Writer(overlaywriter.Writer):
    def tmap(self, base, gain_map, payload, size, colr=None, clli=None, refs=None):
        """refs: raw override of the 'dimg' references (malformed files); colr: (primaries, transfer, matrix, full_range) of the
        alternate rendition; clli: (max_cll, max_pall)"""
        a = [self._prop(_full(b"ispe", 0, 0, struct.pack(">II", *size)))]
        if colr is not None:
            a.append(self._prop(_colr(colr)))
        if clli is not None:
            a.append(self._prop(clli_box(*clli)))
        tid = self._add(b"tmap", payload, a)
        to = [base, gain_map] if refs is None else list(refs)
        if to:
            self.refs.append((b"dimg", tid, to))
        return tid

    def aux(self, picture, size, target, urn, chroma_format=0, bit_depth=8, transforms=None, hidden=True):
        """an auxiliary image of `target` with the auxC URN `urn`"""
        aid = self.hvc1(picture, size, chroma_format, bit_depth, transforms=transforms, hidden=hidden)
        self.assoc[aid].append(0x8000 | self._prop(_full(b"auxC", 0, 0, urn.encode() + b"\0")))
        self.refs.append((b"auxl", aid, [target]))
        return aid
