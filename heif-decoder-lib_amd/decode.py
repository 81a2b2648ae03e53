"""HEIF bytes -> CUDA tensor, without the pixels leaving the device (hm_decode_item_to_device / hm_pipeline_submit_to_device).

    img = decode_to_tensor(open("a.heic", "rb").read())                           # 3 x H x W float32
    batch = decode_batch_to_tensor(files, dtype=torch.float16, scale=1 / 255)     # N x 3 x H x W
    clip = decode_sequence_to_tensor(movie, frames=range(1, 65, 4), size=(224, 224))   # 16 x 3 x 224 x 224
    crops = decode_to_views(data, [(c, (96, 96)) for c in boxes])                 # a list of 3 x 96 x 96: ONE decode, many crops

Layouts: "chw" (one plane per channel) and "hwc" (the target's own interleaving).  dtypes: torch.uint8 / torch.uint16 (must be
the target's own sample type: 8-bit "rgb" / "rgba", 16-bit "rrggbb_le" / "rrggbbaa_le" ...), torch.float16, torch.float32;
floats are sample * scale[c] + bias[c], rounded after each step.  crop=(x, y, w, h) and size=(w, h) ask for a rectangle of the image,
resampled (filter "triangle": antialiased bilinear, "bicubic", "lanczos3" or "nearest") in the step that writes the tensor; of a grid only the tiles the
rectangle touches are decoded.  light=True asks for linear light (the image's own transfer function undone by a table, floats only);
light=dict(to_transfer="srgb", to_primaries="bt709", gain=1.0, from_transfer=..., from_primaries=...) re-encodes or changes the
primaries - a resize under light= averages light, not code values.  light={"from": "icc", ...} reads the code values through the item's
ICC profile (a matrix/TRC profile: a phone's Display P3) instead of its nclx codes.  tone=dict(dst_peak=203.0, src_peak=None, unit_nits=None,
out_unit_nits=None, out_bits=None) beside light= maps the content's peak (None: the file's clli / mdcv, else 1000 cd/m2) to the
display's with the BT.2390 curve; out_bits=8 finishes a deeper image in 8-bit codes (torch.uint8 is then accepted for it).
tone=dict(dst_peak=203.0, src_peak="measured", percentile=0.9999) measures the content's peak on the decoded pixels instead (the
single-item call only); measure_light(data) and measure_light_of_tensor(pixels, bits, light) return the numbers themselves, a
LightStats: the histogram over the tone step's 2048 PQ codes of max(R, G, B), the largest norm, percentiles, the average.
alpha="straight" / "premultiplied" / dict(mode="matte", background=(r, g, b)) with out_format "rgba" / "rrggbbaa_le" uses the alpha
channel: a resize sums colour times alpha (no dark fringes around a cut-out), and the tensor holds straight colour, premultiplied
colour, or - three channels - the picture over the background colour (code values at the target's sample depth).
gain=dict(headroom=2.0) beside light= renders an SDR image with a gain map (an ISO 21496-1 'tmap' item: item_id is that item, or its
base image) for a display whose peak is 2 ** headroom times SDR white (math.inf: the full HDR rendition); with
gain=dict(headroom=..., map_item=id, alternate_headroom=..., map_max=..., ...) any image of the file is the map (a vendor gain map
among the auxiliary images, its parameters read elsewhere).
ootf=1000 (or dict(display_peak=1000, gamma=None)) beside light= renders an HLG image's scene light for a display of that peak with
the reference OOTF of BT.2100 (gamma None: the system gamma of the peak); a tone= behind it then takes the display's peak as the
content's and as its unit, so light=dict(to_transfer="srgb", to_primaries="bt709"), ootf=1000, tone=dict(dst_peak=203, out_bits=8)
turns a 10-bit HLG BT.2020 photograph into an sRGB uint8 tensor in one call.
What the library refuses raises capi.HmError.

Planar YCbCr stays planar: decode_to_planes / decode_sequence_to_planes / decode_batch_to_planes return (Y, Cb, Cr[, A]) ("planar":
I420 and its kin) or (Y, CbCr[, A]) ("semiplanar": NV12, P010 with msb_aligned=True) as coded or at the chroma format asked for.

    y, cbcr = decode_to_planes(data, chroma="420", layout="semiplanar")           # NV12: H x W, Hc x Wc x 2, uint8"""
import ctypes as C
import os

from . import capi

OUT_FORMATS = {"rgb": capi.HM_OUT_RGB, "rgba": capi.HM_OUT_RGBA, "rrggbb_le": capi.HM_OUT_RRGGBB_LE, "rrggbb_be": capi.HM_OUT_RRGGBB_BE,
               "rrggbbaa_le": capi.HM_OUT_RRGGBBAA_LE, "rrggbbaa_be": capi.HM_OUT_RRGGBBAA_BE}
LAYOUTS = {"hwc": capi.HM_DEV_LAYOUT_HWC, "chw": capi.HM_DEV_LAYOUT_CHW}
FILTERS = {"triangle": capi.HM_VIEW_TRIANGLE, "nearest": capi.HM_VIEW_NEAREST, "bicubic": capi.HM_VIEW_CUBIC, "lanczos3": capi.HM_VIEW_LANCZOS3}


def _out_format(out_format):
    if isinstance(out_format, str):
        if out_format.lower() not in OUT_FORMATS:
            raise ValueError(f"out_format {out_format!r}: one of {sorted(OUT_FORMATS)}")
        return OUT_FORMATS[out_format.lower()]
    return int(out_format)


def _dtype_code(dtype):
    import torch
    codes = {torch.uint8: capi.HM_DEV_U8, torch.uint16: capi.HM_DEV_U16, torch.float16: capi.HM_DEV_F16, torch.float32: capi.HM_DEV_F32}
    if dtype not in codes:
        raise ValueError(f"dtype {dtype}: one of torch.uint8, torch.uint16, torch.float16, torch.float32")
    return codes[dtype]


def _channels(fmt):
    L = capi.image_lib()
    obpp = capi.check_image(L.hm_out_bytes_per_pixel(fmt))
    return obpp // (2 if obpp >= 6 else 1)


def _per_channel(v, default):
    if v is None:
        v = default
    if isinstance(v, (int, float)):
        v = [float(v)] * 4
    v = [float(x) for x in v]
    if not 1 <= len(v) <= 4:
        raise ValueError("scale / bias: a number or up to four per-channel values")
    return v + [default] * (4 - len(v))


def _layout(layout):
    if str(layout).lower() not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'chw' or 'hwc'")
    return LAYOUTS[str(layout).lower()]


def _shape(layout, c, h, w):
    return (c, h, w) if layout == capi.HM_DEV_LAYOUT_CHW else (h, w, c)


def _dest_of(t, layout, dtype_code, c, scale, bias):
    """hm_device_dest of one image-shaped view `t` (C x H x W or H x W x C): its strides become the pitches"""
    es = t.element_size()
    if layout == capi.HM_DEV_LAYOUT_CHW:
        ok = t.stride(2) == 1 or t.shape[2] == 1
        row, plane = t.stride(1) * es, t.stride(0) * es
    else:
        ok = (t.stride(2) == 1 or t.shape[2] == 1) and (t.stride(1) == c or t.shape[1] == 1)
        row, plane = t.stride(0) * es, 0
    if not ok or row < 0 or plane < 0:
        raise ValueError("out: the pixels of a row must be contiguous (only the row and plane strides are free)")
    d = capi.DeviceDest()
    d.ptr = t.data_ptr()
    d.len = t.untyped_storage().nbytes() - t.storage_offset() * es
    d.layout, d.dtype = layout, dtype_code
    d.row_pitch, d.plane_pitch = row, plane
    for k in range(4):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    return d


def _view_of(crop, size, filter, w, h):
    """(hm_device_view or None, width, height written) for an image of w x h"""
    if crop is None and size is None:
        return None, w, h
    if str(filter).lower() not in FILTERS:
        raise ValueError(f"filter {filter!r}: one of {sorted(FILTERS)}")
    v = capi.DeviceView()
    v.filter = FILTERS[str(filter).lower()]
    if crop is not None:
        x, y, cw, ch = (int(t) for t in crop)
        if cw <= 0 or ch <= 0:
            raise ValueError(f"crop {tuple(crop)}: (x, y, w, h) with a positive extent")
        v.crop_x, v.crop_y, v.crop_w, v.crop_h = x, y, cw, ch
        w, h = cw, ch
    if size is not None:
        ow, oh = (int(t) for t in size)
        if ow <= 0 or oh <= 0:
            raise ValueError(f"size {tuple(size)}: (w, h) with a positive extent")
        v.out_w, v.out_h = ow, oh
        w, h = ow, oh
    return v, w, h


TRANSFERS = {"linear": 8, "srgb": 13, "bt709": 1, "pq": 16, "hlg": 18}
PRIMARIES = {"bt709": 1, "srgb": 1, "bt2020": 9, "p3": 12}


def _light_of(light):
    """hm_device_light (or None) of the light= argument: True, or a dict of to_transfer / to_primaries / gain / from_transfer /
    from_primaries with H.273 codes or names; "from": "icc" (or "icc" as the value of from_transfer / from_primaries) makes the item's ICC
    profile the source - the library refuses it set in one of the two only"""
    if light is None or light is False:
        return None
    if light is True:
        light = {}
    if not isinstance(light, dict):
        raise ValueError(f"light {light!r}: True or a dict")
    keys = {"to_transfer", "to_primaries", "gain", "from_transfer", "from_primaries", "from"}
    if set(light) - keys:
        raise ValueError(f"light: unknown keys {sorted(set(light) - keys)}, known are {sorted(keys)}")

    if "from" in light:
        if light["from"] != "icc":
            raise ValueError(f"light['from'] = {light['from']!r}: 'icc' (codes go to from_transfer / from_primaries)")
        if "from_transfer" in light or "from_primaries" in light:
            raise ValueError("light: 'from' beside from_transfer / from_primaries")
        light = dict(light, from_transfer="icc", from_primaries="icc")
        del light["from"]

    def code(key, names, default):
        v = light.get(key, default)
        if isinstance(v, str):
            if v.lower() == "icc" and key.startswith("from_"):
                return capi.HM_LIGHT_FROM_ICC
            if v.lower() not in names:
                raise ValueError(f"light[{key!r}] = {v!r}: one of {sorted(names)} or an H.273 code")
            return names[v.lower()]
        return int(v)
    d = capi.DeviceLight()
    d.from_transfer, d.from_primaries = code("from_transfer", TRANSFERS, 0), code("from_primaries", PRIMARIES, 0)
    d.to_transfer, d.to_primaries = code("to_transfer", TRANSFERS, capi.HM_LIGHT_LINEAR), code("to_primaries", PRIMARIES, 0)
    d.gain = float(light.get("gain", 1.0))
    return d


def _tone_of(tone, lit):
    """hm_device_tone (or None) of the tone= argument: a dict of dst_peak (needed) / src_peak / unit_nits / out_unit_nits / out_bits,
    None standing for the library's default; needs a light step"""
    if tone is None or tone is False:
        return None
    if not isinstance(tone, dict):
        raise ValueError(f"tone {tone!r}: a dict")
    keys = {"dst_peak", "src_peak", "unit_nits", "out_unit_nits", "out_bits"}
    if set(tone) - keys:
        raise ValueError(f"tone: unknown keys {sorted(set(tone) - keys)}, known are {sorted(keys)}")
    if lit is None:
        raise ValueError("tone: needs light= (the curve acts on linear light)")
    if tone.get("dst_peak") is None:
        raise ValueError("tone: dst_peak (cd/m2 of the display's peak) is needed")
    d = capi.DeviceTone()
    d.curve = capi.HM_TONE_BT2390
    d.dst_peak = float(tone["dst_peak"])
    for key in ("src_peak", "unit_nits", "out_unit_nits"):
        v = tone.get(key)
        if v is not None and float(v) == 0.0:
            raise ValueError(f"tone[{key!r}] = {v!r}: None asks for the default")
        setattr(d, key, 0.0 if v is None else float(v))
    d.out_bits = 0 if tone.get("out_bits") is None else int(tone["out_bits"])
    return d


def _measured_of(tone):
    """(the tone= argument without what asks for a measured peak, the percentile's fraction or None): src_peak="measured" asks for the
    content's peak to be measured on the decoded pixels (hm_decode_item_to_device_measured), percentile= (default 0.9999) is the share
    of the pixels that peak covers; percentile is accepted only beside it"""
    if not isinstance(tone, dict) or ("percentile" not in tone and not isinstance(tone.get("src_peak"), str)):
        return tone, None
    if tone.get("src_peak") != "measured":
        if isinstance(tone.get("src_peak"), str):
            raise ValueError(f"tone['src_peak'] = {tone['src_peak']!r}: cd/m2, None (the file's own) or 'measured'")
        raise ValueError("tone: percentile is accepted only beside src_peak='measured'")
    p = tone.get("percentile")
    fraction = 0.9999 if p is None else float(p)
    if not (fraction > 0.0 and fraction <= 1.0):
        raise ValueError(f"tone['percentile'] = {p!r}: a fraction in (0, 1]")
    rest = {k: v for k, v in tone.items() if k != "percentile"}
    rest["src_peak"] = None
    return rest, fraction


def _no_measuring(tone):
    """the batch and sequence calls: a tone= that asks for a measured peak is refused"""
    if _measured_of(tone)[1] is not None:
        raise ValueError("tone: src_peak='measured' - only the single-item call (decode_to_tensor) measures; measure_light gives a clip's or a batch's numbers")


def _ootf_of(ootf, lit):
    """hm_device_ootf (or None) of the ootf= argument: a number (the display's peak in cd/m2) or a dict of display_peak (needed) /
    gamma (None: the system gamma of that peak); needs a light step"""
    if ootf is None or ootf is False:
        return None
    if isinstance(ootf, bool):
        raise ValueError(f"ootf {ootf!r}: the display's peak in cd/m2, or a dict")
    if isinstance(ootf, (int, float)):
        ootf = {"display_peak": ootf}
    if not isinstance(ootf, dict):
        raise ValueError(f"ootf {ootf!r}: the display's peak in cd/m2, or a dict")
    keys = {"display_peak", "gamma"}
    if set(ootf) - keys:
        raise ValueError(f"ootf: unknown keys {sorted(set(ootf) - keys)}, known are {sorted(keys)}")
    if lit is None:
        raise ValueError("ootf: needs light= (the OOTF acts on scene light)")
    if ootf.get("display_peak") is None:
        raise ValueError("ootf: display_peak (cd/m2 of the display's peak) is needed")
    d = capi.DeviceOotf()
    d.kind = capi.HM_OOTF_HLG
    d.display_peak = float(ootf["display_peak"])
    g = ootf.get("gamma")
    if g is not None and float(g) == 0.0:
        raise ValueError(f"ootf['gamma'] = {g!r}: None asks for the system gamma")
    d.gamma = 0.0 if g is None else float(g)
    return d


def _ref(s):
    """a ctypes struct by reference, None as a null pointer"""
    return C.byref(s) if s is not None else None


ALPHA_MODES = {"straight": capi.HM_ALPHA_STRAIGHT, "premultiplied": capi.HM_ALPHA_PREMULTIPLIED, "matte": capi.HM_ALPHA_MATTE}


def _alpha_of(alpha, fmt):
    """(hm_device_alpha or None, channels of the tensor) of the alpha= argument for the target fmt: "straight", "premultiplied", or a
    dict of mode and - for "matte" - background=(r, g, b), code values at the target's sample depth; a matte has three channels"""
    if alpha is None or alpha is False:
        return None, _channels(fmt)
    if isinstance(alpha, str):
        alpha = {"mode": alpha}
    if not isinstance(alpha, dict):
        raise ValueError(f"alpha {alpha!r}: 'straight', 'premultiplied' or a dict")
    keys = {"mode", "background"}
    if set(alpha) - keys:
        raise ValueError(f"alpha: unknown keys {sorted(set(alpha) - keys)}, known are {sorted(keys)}")
    mode = alpha.get("mode")
    if not isinstance(mode, str) or mode.lower() not in ALPHA_MODES:
        raise ValueError(f"alpha: mode {mode!r}: one of {sorted(ALPHA_MODES)}")
    if _channels(fmt) != 4:
        raise ValueError("alpha: needs a four-channel out_format ('rgba', 'rrggbbaa_le')")
    d = capi.DeviceAlpha()
    d.mode = ALPHA_MODES[mode.lower()]
    bg = alpha.get("background")
    if d.mode == capi.HM_ALPHA_MATTE:
        if bg is None or len(tuple(bg)) != 3:
            raise ValueError("alpha: a matte needs background=(r, g, b)")
        for k, v in enumerate(bg):
            if isinstance(v, bool) or not hasattr(v, "__index__") or not 0 <= v.__index__() <= 65535:
                raise ValueError(f"alpha: background[{k}] = {v!r}: a code value at the target's sample depth")
            d.background[k] = v.__index__()
    elif bg is not None:
        raise ValueError(f"alpha: background with mode {mode!r} (a matte takes one)")
    return d, 3 if d.mode == capi.HM_ALPHA_MATTE else 4


GAIN_FIELDS = ("map_min", "map_max", "gamma", "base_offset", "alternate_offset")


def _gain_of(gain, lit):
    """hm_device_gain (or None) of the gain= argument: a dict of headroom (needed; log2(display peak / SDR white), math.inf allowed) and
    optionally map_item with the explicit parameters base_headroom, alternate_headroom, map_min, map_max, gamma, base_offset,
    alternate_offset (a number for all three channels or three numbers) and use_base_primaries; needs a light step"""
    if gain is None or gain is False:
        return None
    if not isinstance(gain, dict):
        raise ValueError(f"gain {gain!r}: a dict")
    keys = {"headroom", "map_item", "base_headroom", "alternate_headroom", "use_base_primaries"} | set(GAIN_FIELDS)
    if set(gain) - keys:
        raise ValueError(f"gain: unknown keys {sorted(set(gain) - keys)}, known are {sorted(keys)}")
    if lit is None:
        raise ValueError("gain: needs light= (the gain acts on linear light)")
    if gain.get("headroom") is None:
        raise ValueError("gain: headroom (log2 of the display's peak over SDR white) is needed")
    d = capi.DeviceGain()
    d.headroom = float(gain["headroom"])
    explicit = sorted(k for k in keys - {"headroom", "map_item"} if gain.get(k) is not None)
    if not gain.get("map_item"):
        if explicit:
            raise ValueError(f"gain: {explicit} without map_item (a 'tmap' item brings its own parameters)")
        return d
    d.map_item = int(gain["map_item"])
    p = d.params
    p.base_headroom = float(gain.get("base_headroom") or 0.0)
    if gain.get("alternate_headroom") is None:
        raise ValueError("gain: map_item needs the explicit parameters, alternate_headroom among them")
    p.alternate_headroom = float(gain["alternate_headroom"])
    defaults = {"map_min": 0.0, "map_max": None, "gamma": 1.0, "base_offset": 1.0 / 64.0, "alternate_offset": 1.0 / 64.0}
    for key in GAIN_FIELDS:
        v = gain.get(key, defaults[key])
        if v is None:
            raise ValueError(f"gain: map_item needs the explicit parameters, {key} among them")
        v = [float(v)] * 3 if not hasattr(v, "__len__") else [float(x) for x in v]
        if len(v) != 3:
            raise ValueError(f"gain[{key!r}]: one number or three")
        for c in range(3):
            getattr(p, key)[c] = v[c]
    p.use_base_primaries = 1 if gain.get("use_base_primaries", True) else 0
    return d


class _Steps:
    """The steps of a request for the target fmt: alp and c (the channels of the tensor) from the alpha= argument at once, lit, ton, gn
    and oo from light=, tone=, gain= and ootf= where the caller parses them (parse) - ctypes structs or None.  What does not go together
    is refused there."""

    def __init__(self, alpha, fmt):
        self.alp, self.c = _alpha_of(alpha, fmt)
        self.lit = self.ton = self.gn = self.oo = self.fraction = None

    def parse(self, light, tone, gain, ootf, measures=False):
        """measures: the caller is the single-item call, which can measure the content's peak (tone's src_peak="measured")"""
        self.lit = _light_of(light)
        if not measures:
            _no_measuring(tone)
        tone, self.fraction = _measured_of(tone)
        self.ton = _tone_of(tone, self.lit)
        if self.fraction is not None and (self.alp is not None or gain is not None):
            raise ValueError("tone: src_peak='measured' beside alpha= or gain= (the measured entry takes view, light, ootf and tone)")
        self.gn = _gain_of(gain, self.lit)
        self.oo = _ootf_of(ootf, self.lit)
        if self.gn is not None and self.alp is not None:
            raise capi.HmError(-2, "gain: an alpha step beside the gain step is not supported (the open step)")
        if self.gn is not None and self.oo is not None:
            raise capi.HmError(-2, "ootf: a gain step beside the OOTF step is not supported (a gain map's base is SDR)")
        return self

    def entry(self, L, family, view):
        """(the entry of `family` - hm_decode_item_to_device, hm_decode_frames_to_device, hm_pipeline_submit_to_device - this request with
        `view` (or None) goes through, its step arguments in the entry's order): capi.ENTRY_KINDS"""
        return _entry(L, family, dict(view=view, light=self.lit, tone=self.ton, alpha=self.alp, gain=self.gn, ootf=self.oo))


def _entry(L, family, steps, planes=False):
    name, args = capi.entry_of(family, {k for k, v in steps.items() if v is not None}, planes)
    return getattr(L, name), [_ref(steps[a]) for a in args]


def _gain_items(f, iid, gn):
    """(the item the decode is asked for, the item whose size the tensor has): a 'tmap' item and its base image - iid itself when it
    is a 'tmap' item, else the 'tmap' item whose base iid is (hm_file_gain_map_of) -, or with an explicit map_item iid twice"""
    L = f.L
    if gn.map_item:
        return iid, iid
    tmap = iid if L.hm_file_item_kind(f.h, iid) == capi.HM_ITEM_TMAP else L.hm_file_gain_map_of(f.h, iid)
    if not tmap:
        raise ValueError(f"gain: item {iid} is no 'tmap' item and no 'tmap' item has it as its base image (give map_item and the parameters)")
    info = capi.GainMapInfo()
    capi.check_image(L.hm_file_gain_map_info(f.h, tmap, C.byref(info)))
    return tmap, info.base_item


def _default_threads():
    return max(1, min(16, os.cpu_count() or 1))


class _File:
    def __init__(self, data):
        self.L = capi.image_lib()
        self.h = C.c_void_p()
        capi.check_image(self.L.hm_file_open(data, len(data), C.byref(self.h)))

    def size(self, item_id):
        iid = item_id or self.L.hm_file_primary_item(self.h)
        info = capi.ImageInfo()
        capi.check_image(self.L.hm_file_image_info(self.h, iid, C.byref(info)))
        return iid, info.width, info.height

    def close(self):
        if self.h:
            self.L.hm_file_close(self.h)
            self.h = C.c_void_p()


def decode_to_tensor(data, item_id=0, out_format="rgb", layout="chw", dtype=None, scale=None, bias=None, out=None, stream=None,
                     host_threads=None, crop=None, size=None, filter="triangle", light=None, tone=None, alpha=None, gain=None, ootf=None):
    """Decode one image of a HEIF file (bytes; item_id 0 = the primary item) into a CUDA tensor: C x H x W ("chw") or H x W x C
    ("hwc").  dtype defaults to torch.float32 (out's dtype when out is given).  out: a CUDA tensor of that shape to write into;
    its row (and plane) stride is honoured, bytes between rows are left alone.  stream: a torch.cuda.Stream or a raw stream
    handle (default: the current stream).  crop: (x, y, w, h), a rectangle of the image; size: (w, h), what it is resampled to
    (H and W of the tensor are then the size's, or the crop's); filter: "triangle", "bicubic", "lanczos3" or "nearest".  light: True (linear
    light) or a dict (see the module's text): the light step in the write of the tensor; tone: a dict (see the module's text), the tone
    step inside it; alpha: "straight", "premultiplied" or dict(mode="matte", background=(r, g, b)) (see the module's text), the alpha step,
    for a four-channel out_format - a matte gives a tensor of 3 channels.  gain: dict(headroom=...) beside light= (see the module's
    text), the gain step: the image with its gain map for a display of that headroom - item_id may be the 'tmap' item or its base
    image; with map_item and the explicit parameters any image of the file is the map.  ootf: the display's peak in cd/m2 or
    dict(display_peak=..., gamma=None) beside light= (see the module's text), the OOTF step for an HLG image.  Returns when the pixels
    are in place.  Uncompressed ('unci') items are taken like any image - an R G B item to the targets of its own depth ("rgb" / "rgba"
    from 8-bit components, "rrggbb_le" / "rrggbbaa_le" from 16-bit ones); under crop= only the internal tiles it touches are unpacked."""
    import torch
    L = capi.image_lib()
    fmt, lay = _out_format(out_format), _layout(layout)
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    code = _dtype_code(dtype)
    st = _Steps(alpha, fmt)
    c = st.c
    f = _File(data)
    try:
        st.parse(light, tone, gain, ootf, measures=True)
        iid = item_id or L.hm_file_primary_item(f.h)
        sized = iid
        if st.gn is not None:
            iid, sized = _gain_items(f, iid, st.gn)
        _, w, h = f.size(sized)
        view, w, h = _view_of(crop, size, filter, w, h)
        shape = _shape(lay, c, h, w)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device="cuda")
        else:
            if not out.is_cuda or out.dtype != dtype:
                raise ValueError(f"out: a CUDA tensor of dtype {dtype} is needed, got {out.dtype} on {out.device}")
            if tuple(out.shape) != shape:
                raise ValueError(f"out: shape {tuple(out.shape)} does not match the image's {shape}")
        dest = _dest_of(out, lay, code, c, _per_channel(scale, 1.0), _per_channel(bias, 0.0))
        prm = capi.DecodeParams(fmt, host_threads or _default_threads(), 0, 0, _stream_handle(stream, out.device), None, 0, 0, 0, 0)
        d = capi.Decoded()
        fn, steps = st.entry(L, "hm_decode_item_to_device", view)
        with torch.cuda.device(out.device):
            if st.fraction is not None:  # the content's peak measured on the decoded pixels, in the same call
                capi.check_image(L.hm_decode_item_to_device_measured(f.h, iid, C.byref(prm), _ref(view), _ref(st.lit), _ref(st.oo), _ref(st.ton), st.fraction,
                                                                     C.byref(dest), C.byref(d), None))
            else:
                capi.check_image(fn(f.h, iid, C.byref(prm), *steps, C.byref(dest), C.byref(d)))
        if (d.width, d.height) != (w, h):  # (the library checked the destination against the decoded size: nothing else was written)
            raise capi.HmError(-3, f"the decoded image is {d.width} x {d.height}, the file declares {w} x {h}")
        L.hm_decoded_free(C.byref(d))
        return out
    finally:
        f.close()


def decode_to_views(data, views, item_id=0, out_format="rgb", layout="chw", dtype=None, scale=None, bias=None, out=None, stream=None,
                    host_threads=None, filter="triangle", light=None, tone=None, alpha=None, ootf=None, gain=None):
    """Many views of ONE image from ONE decode (hm_decode_item_to_device_views): the crops of a multi-crop training step, the thumbnail
    sizes of one upload, the face rectangles of a region item.  views: a list of (crop, size) or (crop, size, filter) - crop (x, y, w, h)
    and size (w, h) as in decode_to_tensor, either may be None; filter defaults to the call's.  Returns a list of CUDA tensors, one per
    view, each equal to decode_to_tensor(data, crop=crop, size=size, filter=filter, ...).  out: a list of tensors, one per view, or ONE
    4-D tensor whose slices out[k] are the destinations when every view writes the same size (K x C x H x W: the multi-crop case); the
    destinations must not overlap.  light=, tone=, alpha= and ootf= are decode_to_tensor's and apply to every view; gain= and
    tone=dict(src_peak="measured") are decode_to_tensor's alone.  Of a grid only the tiles the bounding rectangle of all crops touches are
    decoded.

        crops = decode_to_views(data, [(c, (96, 96)) for c in crops_of_regions(read_regions(data), image_size)])   # every face, 96 x 96"""
    import torch
    L = capi.image_lib()
    if gain is not None:
        raise ValueError("gain: decode_to_views takes no gain step - call decode_to_tensor(crop=, size=, gain=) per view")
    if isinstance(tone, dict) and tone.get("src_peak") == "measured":
        raise ValueError("tone: decode_to_views does not measure the content's peak - call decode_to_tensor(crop=, size=, tone=dict(src_peak='measured', ...)) per view")
    views = list(views)
    if not 1 <= len(views) <= capi.HM_VIEWS_MOST:
        raise ValueError(f"views: {len(views)} views, 1 .. {capi.HM_VIEWS_MOST} are taken")
    fmt, lay = _out_format(out_format), _layout(layout)
    if dtype is None:
        first = out[0] if out is not None and len(out) else None
        dtype = first.dtype if first is not None else torch.float32
    code = _dtype_code(dtype)
    st = _Steps(alpha, fmt)
    c = st.c
    f = _File(data)
    try:
        st.parse(light, tone, None, ootf)
        iid, w, h = f.size(item_id)
        n = len(views)
        cviews, shapes = (capi.DeviceView * n)(), []
        for k, spec in enumerate(views):
            if len(spec) not in (2, 3):
                raise ValueError(f"views[{k}]: (crop, size) or (crop, size, filter)")
            v, vw, vh = _view_of(spec[0], spec[1], spec[2] if len(spec) == 3 else filter, w, h)
            if v is None:  # (the whole image at its own size: a view of the crop alone)
                v = capi.DeviceView()
            cviews[k] = v
            shapes.append(_shape(lay, c, vh, vw))
        if out is None:
            outs = [torch.empty(s, dtype=dtype, device="cuda") for s in shapes]
        else:
            if len(out) != n:
                raise ValueError(f"out: {len(out)} destinations for {n} views")
            outs = [out[k] for k in range(n)]
            for k, t in enumerate(outs):
                if not t.is_cuda or t.dtype != dtype:
                    raise ValueError(f"out[{k}]: a CUDA tensor of dtype {dtype} is needed, got {t.dtype} on {t.device}")
                if tuple(t.shape) != shapes[k]:
                    raise ValueError(f"out[{k}]: shape {tuple(t.shape)} does not match the view's {shapes[k]}")
        sc, bs = _per_channel(scale, 1.0), _per_channel(bias, 0.0)
        dests = (capi.DeviceDest * n)(*[_dest_of(t, lay, code, c, sc, bs) for t in outs])
        prm = capi.DecodeParams(fmt, host_threads or _default_threads(), 0, 0, _stream_handle(stream, outs[0].device), None, 0, 0, 0, 0)
        d = (capi.Decoded * n)()
        failed = C.c_int32(-1)
        with torch.cuda.device(outs[0].device):
            capi.check_image(L.hm_decode_item_to_device_views(f.h, iid, C.byref(prm), cviews, dests, n, _ref(st.lit), _ref(st.ton), _ref(st.alp), _ref(st.oo), d,
                                                              C.byref(failed)))
        for k in range(n):
            got, want = (d[k].width, d[k].height), (outs[k].shape[2], outs[k].shape[1]) if lay == capi.HM_DEV_LAYOUT_CHW else (outs[k].shape[1], outs[k].shape[0])
            if got != want:
                raise capi.HmError(-3, f"view {k} wrote {got[0]} x {got[1]}, its tensor is {want[0]} x {want[1]}")
        return outs
    finally:
        f.close()


def crops_of_regions(regions, image_size=None):
    """The bounding rectangles of read_regions() geometry as crops (x, y, w, h), in order: every region of every region item of the list
    (or the regions of one item's dict).  image_size=(w, h): the rectangles are brought from the item's reference space to the image
    (where the two differ) and clipped to it; a region that lies outside, or has no extent, is left out.  Masks count with their
    rectangle, a point as one pixel.

        faces = decode_to_views(data, [(c, (112, 112)) for c in crops_of_regions(read_regions(data), (w, h))])"""
    items = [regions] if isinstance(regions, dict) else list(regions)
    crops = []
    for item in items:
        rw, rh = item["reference_size"]
        for r in item["regions"]:
            t = r["type"]
            if t in ("polygon", "polyline"):
                pts = r["points"]
                if len(pts) == 0:
                    continue
                x0, y0, x1, y1 = int(pts[:, 0].min()), int(pts[:, 1].min()), int(pts[:, 0].max()) + 1, int(pts[:, 1].max()) + 1
            elif t == "ellipse":
                x0, y0, x1, y1 = r["x"] - r["w"], r["y"] - r["h"], r["x"] + r["w"] + 1, r["y"] + r["h"] + 1
            elif t == "point":
                x0, y0, x1, y1 = r["x"], r["y"], r["x"] + 1, r["y"] + 1
            else:
                x0, y0, x1, y1 = r["x"], r["y"], r["x"] + r["w"], r["y"] + r["h"]
            if image_size is not None:
                iw, ih = image_size
                if (rw, rh) != (iw, ih) and rw > 0 and rh > 0:  # the outward rounding of a rectangle scaled from the reference space
                    x0, x1 = x0 * iw // rw, -(-x1 * iw // rw)
                    y0, y1 = y0 * ih // rh, -(-y1 * ih // rh)
                x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, iw), min(y1, ih)
            if x1 > x0 and y1 > y0:
                crops.append((int(x0), int(y0), int(x1 - x0), int(y1 - y0)))
    return crops


class LightStats:
    """The light statistics of a rectangle of pixels (hm_light_stats): pixels, histogram (numpy uint32[2048]: pixels per 11-bit PQ code of
    the norm max(R, G, B)), max_norm (the largest norm, in the light step's units), max_code, max_nits, average_nits, and
    percentile(fraction) -> (code, nits of the upper edge of that code's bin)."""

    def __init__(self, c):
        import numpy as np
        self._c = c
        self.pixels = int(c.pixels)
        self.histogram = np.ctypeslib.as_array(c.hist).astype(np.uint32)
        self.max_norm, self.max_code, self.max_nits, self.average_nits = float(c.max_norm), int(c.max_code), float(c.max_nits), float(c.average_nits)

    def percentile(self, fraction):
        code, nits = C.c_int32(), C.c_float()
        capi.check_image(capi.image_lib().hm_light_stats_percentile(C.byref(self._c), float(fraction), C.byref(code), C.byref(nits)))
        return code.value, nits.value

    def __repr__(self):
        return f"LightStats(pixels={self.pixels}, max_code={self.max_code}, max_nits={self.max_nits:.6g}, average_nits={self.average_nits:.6g})"


def _crop_view(crop):
    """hm_device_view (or None) of a crop alone"""
    if crop is None:
        return None
    return _view_of(crop, None, "triangle", 0, 0)[0]


def _unit_nits(unit_nits):
    if unit_nits is not None and float(unit_nits) == 0.0:
        raise ValueError(f"unit_nits = {unit_nits!r}: None asks for the default")
    return 0.0 if unit_nits is None else float(unit_nits)


def measure_light(data, item_id=0, out_format=None, crop=None, light=True, ootf=None, unit_nits=None, host_threads=None, stream=None):
    """Decode one image of a HEIF file and measure its light levels on the device (hm_decode_item_light_stats): a LightStats of the
    whole image, or of crop=(x, y, w, h) - of a grid only the tiles it touches are decoded.  out_format None: "rgb" for 8-bit items,
    "rrggbb_le" for deeper ones.  light: True or a dict as in decode_to_tensor (to_primaries picks the primaries the norm is taken in);
    ootf: as in decode_to_tensor; unit_nits: cd/m2 that light value 1.0 stands for (None: 10000 for PQ, the display's peak beside ootf=)."""
    import torch
    L = capi.image_lib()
    lit = _light_of(light)
    if lit is None:
        raise ValueError("measure_light: needs light= (the statistic is one of linear light)")
    oo = _ootf_of(ootf, lit)
    unit = _unit_nits(unit_nits)
    view = _crop_view(crop)
    f = _File(data)
    try:
        iid = item_id or L.hm_file_primary_item(f.h)
        if out_format is None:
            info = capi.ImageInfo()
            capi.check_image(L.hm_file_image_info(f.h, iid, C.byref(info)))
            out_format = "rgb" if info.bit_depth <= 8 else "rrggbb_le"
        fmt = _out_format(out_format)
        device = torch.device("cuda", torch.cuda.current_device())
        prm = capi.DecodeParams(fmt, host_threads or _default_threads(), 0, 0, _stream_handle(stream, device), None, 0, 0, 0, 0)
        d, s = capi.Decoded(), capi.LightStatsC()
        capi.check_image(L.hm_decode_item_light_stats(f.h, iid, C.byref(prm), _ref(view), _ref(lit), _ref(oo), unit, C.byref(s), C.byref(d)))
        L.hm_decoded_free(C.byref(d))
        return LightStats(s)
    finally:
        f.close()


def measure_light_of_tensor(pixels, bits, light, ootf=None, unit_nits=None, crop=None, stream=None):
    """The light statistics (hm_light_stats_of_tensor) of interleaved pixels on the device: an H x W x 3 or H x W x 4 CUDA tensor of
    torch.uint8 (bits 8) or torch.uint16 / torch.int16 (bits 9 .. 12) code values; its row stride is honoured.  light: a dict with
    from_transfer and from_primaries (the pixels carry no profile); ootf, unit_nits, crop: as measure_light."""
    import torch
    L = capi.image_lib()
    if not isinstance(pixels, torch.Tensor) or not pixels.is_cuda or pixels.dim() != 3 or pixels.shape[2] not in (3, 4):
        raise ValueError("pixels: an H x W x 3 or H x W x 4 CUDA tensor")
    if pixels.dtype not in (torch.uint8, torch.uint16, torch.int16):
        raise ValueError(f"pixels: dtype {pixels.dtype} is not torch.uint8, torch.uint16 or torch.int16")
    wide = pixels.dtype != torch.uint8
    if (int(bits) > 8) != wide or not 8 <= int(bits) <= 16:
        raise ValueError(f"bits {bits!r} with dtype {pixels.dtype}: 8 for torch.uint8, 9 and more for 16-bit samples")
    h, w, c = pixels.shape
    if h == 0 or w == 0:
        raise ValueError("pixels: an empty tensor")
    if not ((pixels.stride(2) == 1) and (pixels.stride(1) == c or w == 1) and pixels.stride(0) >= 0):
        raise ValueError("pixels: the pixels of a row must be contiguous (only the row stride is free)")
    lit = _light_of(light)
    if lit is None:
        raise ValueError("measure_light_of_tensor: needs light= with from_transfer and from_primaries")
    oo = _ootf_of(ootf, lit)
    unit = _unit_nits(unit_nits)
    view = _crop_view(crop)
    fmt = {(False, 3): capi.HM_OUT_RGB, (False, 4): capi.HM_OUT_RGBA, (True, 3): capi.HM_OUT_RRGGBB_LE, (True, 4): capi.HM_OUT_RRGGBBAA_LE}[(wide, c)]
    s = capi.LightStatsC()
    with torch.cuda.device(pixels.device):
        capi.check_image(L.hm_light_stats_of_tensor(fmt, int(bits), w, h, pixels.data_ptr(), pixels.stride(0) * pixels.element_size(), _ref(view), _ref(lit), _ref(oo),
                                                    unit, C.byref(s), _stream_handle(stream, pixels.device)))
    return LightStats(s)


def decode_batch_to_tensor(files, item_id=0, out_format="rgb", layout="chw", dtype=None, scale=None, bias=None, out=None,
                           host_threads=None, max_in_flight=4, size=None, crops=None, filter="triangle", light=None, tone=None, alpha=None, gain=None,
                           ootf=None):
    """Decode N equally sized HEIF files through ONE hm_pipeline (the entropy decode of one file runs under the kernels of
    another) into one N x C x H x W ("chw") or N x H x W x C ("hwc") CUDA tensor, each image into its slice.  files: bytes
    objects or paths.  A file of another size than the first (or than `out`) raises ValueError naming it.
    size: (w, h) - files of different sizes are accepted then, each resampled into its slice; crops: one (x, y, w, h) or None per
    file, the rectangle of that file that is resampled (needs size).  light, tone, alpha, gain, ootf: as decode_to_tensor, the same steps
    for every file (tone's src_peak None: each file's own, beside ootf= the display's peak; gain: each file's own 'tmap' item)."""
    import torch
    L = capi.image_lib()
    fmt, lay = _out_format(out_format), _layout(layout)
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    code = _dtype_code(dtype)
    st = _Steps(alpha, fmt)
    sc, bi = _per_channel(scale, 1.0), _per_channel(bias, 0.0)
    c, gn = st.c, st.parse(light, tone, gain, ootf).gn
    names, datas = [], []
    for k, entry in enumerate(files):
        if isinstance(entry, (bytes, bytearray, memoryview)):
            names.append(f"files[{k}]")
            datas.append(bytes(entry))
        else:
            names.append(os.fspath(entry))
            with open(entry, "rb") as fh:
                datas.append(fh.read())
    if not datas:
        raise ValueError("files: empty")
    if crops is not None and size is None:
        raise ValueError("crops: needs size (the slices of one tensor are equally sized)")
    if crops is not None and len(crops) != len(datas):
        raise ValueError(f"crops: {len(crops)} entries for {len(datas)} files")
    resized = size is not None
    views = [None] * len(datas)
    ids, size = [], (None if size is None else (int(size[0]), int(size[1])))
    want = size
    if out is not None:
        if out.dim() != 4 or not out.is_cuda or out.dtype != dtype or out.shape[0] != len(datas):
            raise ValueError(f"out: a 4-D CUDA tensor of dtype {dtype} with {len(datas)} images is needed")
        s = tuple(out.shape[1:])
        size = (s[2], s[1]) if lay == capi.HM_DEV_LAYOUT_CHW else (s[1], s[0])
        if s != _shape(lay, c, size[1], size[0]):
            raise ValueError(f"out: shape {tuple(out.shape)} does not hold {c}-channel images in layout {layout!r}")
        if resized and size != want:
            raise ValueError(f"out: shape {tuple(out.shape)} does not hold images of size {want[0]} x {want[1]}")
    for k, (name, data) in enumerate(zip(names, datas)):
        f = _File(data)
        try:
            iid = item_id or L.hm_file_primary_item(f.h)
            sized = iid
            if gn is not None:
                iid, sized = _gain_items(f, iid, gn)
            _, w, h = f.size(sized)
        finally:
            f.close()
        if resized:
            views[k], w, h = _view_of(crops[k] if crops is not None else None, size, filter, w, h)
        if size is None:
            size = (w, h)
        if (w, h) != size:
            raise ValueError(f"{name}: the image is {w} x {h}, the batch is {size[0]} x {size[1]}")
        ids.append(iid)
    if out is None:
        out = torch.empty((len(datas),) + _shape(lay, c, size[1], size[0]), dtype=dtype, device="cuda")
    cfg = capi.PipelineConfig(host_threads or _default_threads(), max(1, int(max_in_flight)), fmt, 0, 0, 0, out.device.index, 0, 0)
    pipe = C.c_void_p()
    with torch.cuda.device(out.device):
        torch.cuda.current_stream().synchronize()  # (the pipeline works on streams of its own: `out` must be ready for them)
        capi.check_image(L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)))
        try:
            def take():
                r = capi.PipelineResult()
                capi.check_image(L.hm_pipeline_next(pipe, C.byref(r)))
                tag, status = r.tag, r.status
                detail = L.hm_last_error().decode() if status else ""
                L.hm_pipeline_release(pipe, C.byref(r))
                if status:
                    raise capi.HmError(status, f"{names[tag]}: {detail}")
            for k, data in enumerate(datas):
                dest = _dest_of(out[k], lay, code, c, sc, bi)
                fn, steps = st.entry(L, "hm_pipeline_submit_to_device", views[k])
                while True:
                    rc = fn(pipe, data, len(data), ids[k], k, *steps, C.byref(dest))
                    if rc < 0:  # refused at submission (e.g. a derived item: the pipeline takes coded images and grids): name the file
                        raise capi.HmError(rc, f"{names[k]}: {L.hm_last_error().decode()}")
                    if rc != capi.HM_PIPELINE_FULL:
                        break
                    take()
            while L.hm_pipeline_pending(pipe):
                take()
        finally:
            L.hm_pipeline_destroy(pipe)
    return out


def _frame_ids(frames, n_frames):
    """the 1-based frame IDs `frames` asks for (None: all, a range, or a list) of a sequence of n_frames"""
    if frames is None:
        ids = list(range(1, n_frames + 1))
    else:
        ids = []
        for k, v in enumerate(frames):
            if isinstance(v, bool) or not hasattr(v, "__index__"):
                raise ValueError(f"frames[{k}] = {v!r}: 1-based frame IDs (integers) are needed")
            v = v.__index__()
            if not 1 <= v <= n_frames:
                raise ValueError(f"frames[{k}] = {v}: the sequence has frames 1..{n_frames}")
            ids.append(v)
    if not ids:
        raise ValueError("frames: empty")
    return ids


def decode_sequence_to_tensor(data, frames=None, out_format="rgb", layout="chw", dtype=None, scale=None, bias=None, out=None, stream=None,
                              host_threads=None, crop=None, size=None, filter="triangle", light=None, tone=None, ootf=None):
    """Decode frames of an image sequence (bytes of a file with a 'moov' track) into one CUDA tensor, T x C x H x W ("chw") or
    T x H x W x C ("hwc"), in ONE device batch (hm_decode_frames_to_device_view).  frames: None (all), a range or a list of 1-based
    frame IDs, in any order, repeats allowed - range(1, n + 1, 4) is every fourth frame.  crop / size / filter: the same rectangle
    of every frame, resampled, as in decode_to_tensor; without them every frame must have the size of the first.  out: a CUDA
    tensor of that shape; the row and plane strides of each of its slices are honoured.  light: as decode_to_tensor, the same step for
    every frame (hm_decode_frames_to_device_light); tone: as decode_to_tensor (a frame carries no light levels: src_peak None is 1000);
    ootf: as decode_to_tensor.  Returns when the pixels are in place."""
    import torch
    L = capi.image_lib()
    fmt, lay = _out_format(out_format), _layout(layout)
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    code = _dtype_code(dtype)
    st = _Steps(None, fmt)
    c = st.c
    _no_measuring(tone)
    sc, bi = _per_channel(scale, 1.0), _per_channel(bias, 0.0)
    f = _File(data)
    try:
        info = capi.SequenceInfo()
        capi.check_image(L.hm_file_sequence_info(f.h, C.byref(info)))
        if not info.is_sequence:
            raise capi.HmError(-1, "the file is not an image sequence")
        ids = _frame_ids(frames, info.frame_count)
        view, w, h = None, None, None
        for k, fid in enumerate(ids):
            _, fw, fh = f.size(fid)
            v, vw, vh = _view_of(crop, size, filter, fw, fh)
            if view is None:
                view, w, h = v, vw, vh
            if (vw, vh) != (w, h):
                raise ValueError(f"frames[{k}] (frame {fid}) is {vw} x {vh}, the first is {w} x {h}: give a size")
        shape = (len(ids),) + _shape(lay, c, h, w)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device="cuda")
        else:
            if tuple(out.shape) != shape:
                raise ValueError(f"out: shape {tuple(out.shape)} does not match the frames' {shape}")
            if not out.is_cuda or out.dtype != dtype:
                raise ValueError(f"out: a CUDA tensor of dtype {dtype} is needed, got {out.dtype} on {out.device}")
        n = len(ids)
        dests = (capi.DeviceDest * n)(*[_dest_of(out[k], lay, code, c, sc, bi) for k in range(n)])
        prm = capi.DecodeParams(fmt, host_threads or _default_threads(), 0, 0, _stream_handle(stream, out.device), None, 0, 0, 0, 0)
        res = (capi.Decoded * n)()
        failed = C.c_int32(-1)
        fn, steps = st.parse(light, tone, None, ootf).entry(L, "hm_decode_frames_to_device", view)
        with torch.cuda.device(out.device):
            rc = fn(f.h, (C.c_uint32 * n)(*ids), n, C.byref(prm), *steps, dests, res, C.byref(failed))
        if rc < 0:
            detail = f"{L.hm_status_string(rc).decode()}: {L.hm_last_error().decode()}"
            k = failed.value
            if k >= 0 and view is None and "device destination:" in detail:
                # a slice shaped for the size the track declares does not hold this frame's picture: find its own size (one host
                # decode, on this path only) and name it
                one = capi.Decoded()
                if L.hm_decode_item(f.h, ids[k], C.byref(prm), C.byref(one)) == 0:
                    fw, fh = one.width, one.height
                    L.hm_decoded_free(C.byref(one))
                    if (fw, fh) != (w, h):
                        raise ValueError(f"frames[{k}] (frame {ids[k]}) is {fw} x {fh}, the track declares {w} x {h}: give a size")
            raise capi.HmError(rc, f"frames[{k}] (frame {ids[k]}): {detail}" if k >= 0 else detail)
        sizes = [(res[k].width, res[k].height) for k in range(n)]
        for k in range(n):
            L.hm_decoded_free(C.byref(res[k]))
        for k in range(n):  # (a track declares one size for all its samples; a smaller picture was written into the corner of its slice)
            if sizes[k] != (w, h):
                raise ValueError(f"frames[{k}] (frame {ids[k]}) is {sizes[k][0]} x {sizes[k][1]}, the track declares {w} x {h}: give a size")
        return out
    finally:
        f.close()


# ---- planar YCbCr (hm_device_planes) -----------------------------------------------------------------------------------------------

PLANE_LAYOUTS = {"planar": capi.HM_DEV_PLANES_SEPARATE, "semiplanar": capi.HM_DEV_PLANES_SEMI}
PLANAR_TARGETS = {None: 0, "420": capi.HM_OUT_YCBCR_420, "422": capi.HM_OUT_YCBCR_422, "444": capi.HM_OUT_YCBCR_444}


def _planes_request(chroma, layout, to_8bit):
    key = None if chroma is None else str(chroma)
    if key not in PLANAR_TARGETS:
        raise ValueError(f"chroma {chroma!r}: None (as coded), '420', '422' or '444'")
    if str(layout).lower() not in PLANE_LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'planar' or 'semiplanar'")
    if to_8bit and key is None:
        raise ValueError("to_8bit: needs a chroma target (the picture as coded keeps its depth)")
    return PLANAR_TARGETS[key], PLANE_LAYOUTS[str(layout).lower()]


def _result_format(info, fmt, to_8bit):
    """(chroma format, bits) of the planar result for a file of hm_image_info `info`: a target that equals the coded format converts nothing"""
    as_coded = fmt == 0 or (info.chroma != 0 and info.chroma == (fmt & 3))
    return (info.chroma, info.bit_depth) if as_coded else (fmt & 3, 8 if to_8bit else info.bit_depth)


def _plane_shapes(chroma, lay, w, h, alpha):
    """shapes of the tensors of one image: Y, then Cb and Cr (or CbCr), then alpha"""
    cw, ch = (w if chroma == 3 else (w + 1) // 2), ((h + 1) // 2 if chroma == 1 else h)
    shapes = [(h, w)]
    if chroma != 0:
        shapes += [(ch, cw, 2)] if lay == capi.HM_DEV_PLANES_SEMI else [(ch, cw), (ch, cw)]
    if alpha:
        shapes.append((h, w))
    return shapes


def _planes_of(tensors, chroma, lay, alpha, code, msb_aligned, scale, bias):
    """hm_device_planes of one image's tensors (as _plane_shapes orders them): their row strides become the pitches"""
    d = capi.DevicePlanes()
    d.layout, d.dtype, d.msb_aligned = lay, code, 1 if msb_aligned else 0
    for k in range(4):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    slots = [0] + ([] if chroma == 0 else [1] if lay == capi.HM_DEV_PLANES_SEMI else [1, 2]) + ([3] if alpha else [])
    for t, slot in zip(tensors, slots):
        es = t.element_size()
        if t.dim() == 3:
            ok = (t.stride(2) == 1) and (t.stride(1) == 2 or t.shape[1] == 1)
        else:
            ok = t.stride(1) == 1 or t.shape[1] == 1
        if not ok or t.stride(0) < 0:
            raise ValueError("out: the elements of a row must be contiguous (only the row stride is free)")
        d.plane[slot].ptr = t.data_ptr()
        d.plane[slot].len = t.untyped_storage().nbytes() - t.storage_offset() * es
        d.plane[slot].row_pitch = t.stride(0) * es if t.shape[0] > 1 else 0
    return d


def _check_out(out, shapes, dtype, lead=()):
    if len(out) != len(shapes):
        raise ValueError(f"out: {len(shapes)} tensors are needed, got {len(out)}")
    for t, shape in zip(out, shapes):
        if not t.is_cuda or t.dtype != dtype:
            raise ValueError(f"out: CUDA tensors of dtype {dtype} are needed, got {t.dtype} on {t.device}")
        if tuple(t.shape) != tuple(lead) + shape:
            raise ValueError(f"out: shape {tuple(t.shape)} does not match the plane's {tuple(lead) + shape}")


def _stream_handle(stream, device):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return (stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)) or None


def _info(f, item_id):
    iid = item_id or f.L.hm_file_primary_item(f.h)
    info = capi.ImageInfo()
    capi.check_image(f.L.hm_file_image_info(f.h, iid, C.byref(info)))
    return iid, info


def _default_plane_dtype(bits):
    import torch
    return torch.uint8 if bits == 8 else torch.uint16


def decode_to_planes(data, item_id=0, chroma=None, layout="planar", dtype=None, to_8bit=False, scale=None, bias=None, out=None, stream=None,
                     host_threads=None, msb_aligned=False, alpha=True, crop=None, size=None, filter="triangle"):
    """Decode one image of a HEIF file into planar YCbCr CUDA tensors: (Y, Cb, Cr[, A]) for layout "planar", (Y, CbCr[, A]) for
    "semiplanar" (a 4:0:0 picture: (Y[, A])).  Y and A are H x W, Cb and Cr Hc x Wc, CbCr Hc x Wc x 2 (Cb first).  chroma: None = as
    coded, "420" / "422" / "444" = converted to that format (to_8bit: down to 8 bits on the way).  dtype defaults to torch.uint8 or
    torch.uint16 by the result's depth (out's dtype when out is given); msb_aligned (torch.uint16): v << (16 - bits), P010.  Floats are
    sample * scale[c] + bias[c], c = Y, Cb, Cr, A.  out: a tuple of CUDA tensors of those shapes; their row strides are honoured.
    The alpha plane is returned when the image has one and alpha is true; alpha=False leaves it out (plane[3] NULL) - the way to an
    integer dtype for an image whose alpha plane is of the other depth class (8 bits beside more than 8), which is refused otherwise.
    crop: (x, y, w, h) inside the image, x (and y for 4:2:0) even where the chroma is sub-sampled; size: (w, h), the luma size every
    plane is resampled for, each plane as an image of its own; filter: as decode_to_tensor.  Only the tiles of a grid the crop touches
    are decoded where the picture is taken as coded.
    An uncompressed ('unci') item of R G B components, taken as coded (chroma=None), returns (R, G, B[, A]), each H x W."""
    import torch
    L = capi.image_lib()
    fmt, lay = _planes_request(chroma, layout, to_8bit)
    sc, bi = _per_channel(scale, 1.0), _per_channel(bias, 0.0)
    f = _File(data)
    try:
        iid, info = _info(f, item_id)
        rchroma, rbits = _result_format(info, fmt, to_8bit)
        alpha = bool(alpha) and bool(info.has_alpha)
        view, w, h = _view_of(crop, size, filter, info.width, info.height)
        if dtype is None:
            dtype = out[0].dtype if out is not None else _default_plane_dtype(rbits)
        code = _dtype_code(dtype)
        shapes = _plane_shapes(rchroma, lay, w, h, alpha)
        if out is None:
            out = tuple(torch.empty(shape, dtype=dtype, device="cuda") for shape in shapes)
        else:
            out = tuple(out)
            _check_out(out, shapes, dtype)
        device = out[0].device
        planes = _planes_of(out, rchroma, lay, alpha, code, msb_aligned, sc, bi)
        prm = capi.DecodeParams(fmt, host_threads or _default_threads(), 0, 0, _stream_handle(stream, device), None, 0, 0, 0, 1 if to_8bit else 0)
        d = capi.Decoded()
        fn, steps = _entry(L, "hm_decode_item_to_device", dict(view=view), planes=True)
        with torch.cuda.device(device):
            capi.check_image(fn(f.h, iid, C.byref(prm), *steps, C.byref(planes), C.byref(d)))
        L.hm_decoded_free(C.byref(d))
        return out
    finally:
        f.close()


def decode_sequence_to_planes(data, frames=None, chroma=None, layout="planar", dtype=None, to_8bit=False, scale=None, bias=None, out=None,
                              stream=None, host_threads=None, msb_aligned=False, crop=None, size=None, filter="triangle"):
    """decode_to_planes over frames of an image sequence in ONE device batch (hm_decode_frames_to_device_planes): a tuple of
    T x ... tensors, frame k in slice k of each.  frames: None (all), a range or a list of 1-based frame IDs, in any order.
    crop / size / filter: the same rectangle of every frame, every plane resampled as an image of its own, in one grouped write
    (hm_decode_frames_to_device_planes_view)."""
    import torch
    L = capi.image_lib()
    fmt, lay = _planes_request(chroma, layout, to_8bit)
    sc, bi = _per_channel(scale, 1.0), _per_channel(bias, 0.0)
    f = _File(data)
    try:
        seq = capi.SequenceInfo()
        capi.check_image(L.hm_file_sequence_info(f.h, C.byref(seq)))
        if not seq.is_sequence:
            raise capi.HmError(-1, "the file is not an image sequence")
        ids = _frame_ids(frames, seq.frame_count)
        first, view = None, None
        for k, fid in enumerate(ids):
            _, info = _info(f, fid)
            v, vw, vh = _view_of(crop, size, filter, info.width, info.height)
            if view is None:
                view = v
            key = (vw, vh) + _result_format(info, fmt, to_8bit)
            if first is None:
                first = key
            if key != first:
                raise ValueError(f"frames[{k}] (frame {fid}) is {key[0]} x {key[1]} (chroma {key[2]}, {key[3]} bits), the first is {first[0]} x {first[1]} "
                                 f"(chroma {first[2]}, {first[3]} bits)")
        w, h, rchroma, rbits = first
        if dtype is None:
            dtype = out[0].dtype if out is not None else _default_plane_dtype(rbits)
        code, n = _dtype_code(dtype), len(ids)
        shapes = _plane_shapes(rchroma, lay, w, h, False)
        if out is None:
            out = tuple(torch.empty((n,) + shape, dtype=dtype, device="cuda") for shape in shapes)
        else:
            out = tuple(out)
            _check_out(out, shapes, dtype, (n,))
        device = out[0].device
        dests = (capi.DevicePlanes * n)(*[_planes_of([t[k] for t in out], rchroma, lay, False, code, msb_aligned, sc, bi) for k in range(n)])
        prm = capi.DecodeParams(fmt, host_threads or _default_threads(), 0, 0, _stream_handle(stream, device), None, 0, 0, 0, 1 if to_8bit else 0)
        res = (capi.Decoded * n)()
        failed = C.c_int32(-1)
        fn, steps = _entry(L, "hm_decode_frames_to_device", dict(view=view), planes=True)
        with torch.cuda.device(device):
            rc = fn(f.h, (C.c_uint32 * n)(*ids), n, C.byref(prm), *steps, dests, res, C.byref(failed))
        if rc < 0:
            detail = f"{L.hm_status_string(rc).decode()}: {L.hm_last_error().decode()}"
            k = failed.value
            raise capi.HmError(rc, f"frames[{k}] (frame {ids[k]}): {detail}" if k >= 0 else detail)
        for k in range(n):
            L.hm_decoded_free(C.byref(res[k]))
        return out
    finally:
        f.close()


def decode_batch_to_planes(files, item_id=0, chroma=None, layout="planar", dtype=None, to_8bit=False, scale=None, bias=None, out=None,
                           host_threads=None, max_in_flight=4, msb_aligned=False, alpha=True, size=None, crops=None, filter="triangle"):
    """decode_to_planes over N files through ONE hm_pipeline: a tuple of N x ... tensors, file k in slice k of each.  files: bytes
    objects or paths.  A file of another size or format (chroma format, depth, alpha) than the first raises ValueError naming it.
    alpha=False: no alpha plane is asked for or returned, and files with and without one go together.
    size: (w, h) - files of different sizes are accepted then, each resampled into its slice; crops: one (x, y, w, h) or None per
    file, the rectangle of that file that is resampled (needs size)."""
    import torch
    L = capi.image_lib()
    fmt, lay = _planes_request(chroma, layout, to_8bit)
    sc, bi = _per_channel(scale, 1.0), _per_channel(bias, 0.0)
    names, datas = [], []
    for k, entry in enumerate(files):
        if isinstance(entry, (bytes, bytearray, memoryview)):
            names.append(f"files[{k}]")
            datas.append(bytes(entry))
        else:
            names.append(os.fspath(entry))
            with open(entry, "rb") as fh:
                datas.append(fh.read())
    if not datas:
        raise ValueError("files: empty")
    if crops is not None and size is None:
        raise ValueError("crops: needs size (the slices of one tensor are equally sized)")
    if crops is not None and len(crops) != len(datas):
        raise ValueError(f"crops: {len(crops)} entries for {len(datas)} files")
    views = [None] * len(datas)
    ids, first = [], None
    for k, (name, data) in enumerate(zip(names, datas)):
        f = _File(data)
        try:
            iid, info = _info(f, item_id)
        finally:
            f.close()
        fw, fh = info.width, info.height
        if size is not None:
            views[k], fw, fh = _view_of(crops[k] if crops is not None else None, size, filter, fw, fh)
        key = (fw, fh) + _result_format(info, fmt, to_8bit) + (bool(alpha) and bool(info.has_alpha),)
        if first is None:
            first = key
        if key != first:
            raise ValueError(f"{name}: the image is {key[0]} x {key[1]} (chroma {key[2]}, {key[3]} bits, alpha {key[4]}), the batch is "
                             f"{first[0]} x {first[1]} (chroma {first[2]}, {first[3]} bits, alpha {first[4]})")
        ids.append(iid)
    w, h, rchroma, rbits, alpha = first
    if dtype is None:
        dtype = out[0].dtype if out is not None else _default_plane_dtype(rbits)
    code, n = _dtype_code(dtype), len(datas)
    shapes = _plane_shapes(rchroma, lay, w, h, alpha)
    if out is None:
        out = tuple(torch.empty((n,) + shape, dtype=dtype, device="cuda") for shape in shapes)
    else:
        out = tuple(out)
        _check_out(out, shapes, dtype, (n,))
    device = out[0].device
    cfg = capi.PipelineConfig(host_threads or _default_threads(), max(1, int(max_in_flight)), fmt | (capi.HM_OUT_YCBCR_8BIT if to_8bit else 0), 0, 0, 0,
                              device.index, 0, 0)
    pipe = C.c_void_p()
    with torch.cuda.device(device):
        torch.cuda.current_stream().synchronize()  # (the pipeline works on streams of its own: `out` must be ready for them)
        capi.check_image(L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)))
        try:
            def take():
                r = capi.PipelineResult()
                capi.check_image(L.hm_pipeline_next(pipe, C.byref(r)))
                tag, status = r.tag, r.status
                detail = L.hm_last_error().decode() if status else ""
                L.hm_pipeline_release(pipe, C.byref(r))
                if status:
                    raise capi.HmError(status, f"{names[tag]}: {detail}")
            for k, data in enumerate(datas):
                planes = _planes_of([t[k] for t in out], rchroma, lay, alpha, code, msb_aligned, sc, bi)
                fn, steps = _entry(L, "hm_pipeline_submit_to_device", dict(view=views[k]), planes=True)
                while True:
                    rc = capi.check_image(fn(pipe, data, len(data), ids[k], k, *steps, C.byref(planes)))
                    if rc != capi.HM_PIPELINE_FULL:
                        break
                    take()
            while L.hm_pipeline_pending(pipe):
                take()
        finally:
            L.hm_pipeline_destroy(pipe)
    return out


# ---- regions and masks: what a file says about its pixels ('rgan' region items, 'mski' mask items) ----

REGION_MODES = {"stack": capi.HM_REGIONS_STACK, "labels": capi.HM_REGIONS_LABELS}


def _region_item_ids(f, iid, region_items):
    L = f.L
    if region_items is not None:
        return [int(r) for r in region_items]
    n = capi.check_image(L.hm_file_region_items(f.h, iid, None, 0))
    ids = (C.c_uint32 * max(n, 1))()
    capi.check_image(L.hm_file_region_items(f.h, iid, ids, n))
    return [ids[i] for i in range(n)]


def _read_region_item(f, rid):
    import numpy as np
    L = f.L
    info = capi.RegionItemInfo()
    capi.check_image(L.hm_file_region_item_info(f.h, rid, C.byref(info)))
    regions = []
    for k in range(info.n_regions):
        g = capi.Region()
        capi.check_image(L.hm_file_region(f.h, rid, k, C.byref(g)))
        pts = np.zeros((g.n_points, 2), dtype=np.int32)
        if g.n_points:
            capi.check_image(L.hm_file_region_points(f.h, rid, k, pts.ctypes.data_as(C.POINTER(C.c_int32)), g.n_points))
        r = dict(type=capi.REGION_TYPE_NAMES[g.type], x=g.x, y=g.y, w=g.w, h=g.h, points=pts, mask_item=g.mask_item)
        if g.type == capi.HM_REGION_INLINE_MASK:
            p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
            capi.check_image(L.hm_file_region_inline_mask(f.h, rid, k, C.byref(p), C.byref(n)))
            r["bits"] = C.string_at(p, n.value)
        regions.append(r)
    return dict(item_id=rid, reference_size=(info.reference_width, info.reference_height), regions=regions)


def read_regions(data, item_id=0):
    """The region items ('rgan') that annotate image item_id (0 = the primary item) of a HEIF file, in item-id order: a list of
    dict(item_id=, reference_size=(w, h), regions=[...]), each region a dict(type= "point" / "rectangle" / "ellipse" / "polygon" /
    "referenced_mask" / "inline_mask" / "polyline", x=, y=, w=, h= (an ellipse: centre and radii), points= an N x 2 int32 array,
    mask_item= the mask item of a referenced mask (else 0), and for an inline mask bits= its bit string).  Host only: no GPU is needed.
    A damaged region item raises capi.HmError."""
    f = _File(data)
    try:
        iid = item_id or f.L.hm_file_primary_item(f.h)
        return [_read_region_item(f, rid) for rid in _region_item_ids(f, iid, None)]
    finally:
        f.close()


def _regions_view(reference_size, image_size, crop, size, filter):
    """(hm_device_view or None, width, height written) of a region raster: crop is in the reference space; with neither crop nor size
    and a reference size that differs from the image's, size defaults to the image's - the planes then line up with decode_to_tensor"""
    rw, rh = reference_size
    if tuple(reference_size) != tuple(image_size):
        if crop is not None and size is None:
            raise ValueError(f"crop without size: the regions' reference space is {rw} x {rh}, the image {image_size[0]} x {image_size[1]} - a crop is in "
                             "the reference space, so say which size it is to be written at (size=(w, h))")
        if crop is None and size is None:
            size = tuple(image_size)
    return _view_of(crop, size, filter, rw, rh)


def decode_regions_to_tensor(data, item_id=0, region_items=None, mode="stack", crop=None, size=None, filter="triangle", dtype=None, scale=None,
                             bias=None, out=None, stream=None):
    """Rasterise the regions that annotate image item_id (0 = the primary item) into a CUDA tensor: R x H x W for mode "stack" (one
    plane per region, 0 / 255, a referenced mask its samples) or H x W uint8 for "labels" (1 + the index of the last region whose value
    is >= 128, else 0).  region_items: ids of the region items to take (None: all of the image's, in item-id order; they must share one
    reference size).  crop: (x, y, w, h) in the regions' reference space; size: (w, h) written - "stack" planes are resampled with
    `filter` like the planes of decode_to_planes, "labels" takes filter="nearest" only.  With neither, and a reference size that differs
    from the image's, size defaults to the image's size, so that the planes line up pixel for pixel with decode_to_tensor; with a crop
    in that case size must be given (ValueError).  dtype: torch.uint8 (the default), torch.float16 / torch.float32 ("stack": value *
    scale + bias).  out: a CUDA tensor of that shape; its row and plane strides are honoured.  stream: work queued on it is waited for
    first; the call returns when the planes are in place."""
    import torch
    L = capi.image_lib()
    if str(mode).lower() not in REGION_MODES:
        raise ValueError(f"mode {mode!r}: 'stack' or 'labels'")
    m = REGION_MODES[str(mode).lower()]
    if dtype is None:
        dtype = out.dtype if out is not None else torch.uint8
    code = _dtype_code(dtype)
    f = _File(data)
    try:
        iid, iw, ih = f.size(item_id)
        ids = _region_item_ids(f, iid, region_items)
        if not ids:
            raise ValueError(f"item {iid} has no region items")
        n = 0
        ref = None
        for rid in ids:
            info = capi.RegionItemInfo()
            capi.check_image(L.hm_file_region_item_info(f.h, rid, C.byref(info)))
            n += info.n_regions
            ref = ref or (info.reference_width, info.reference_height)
        view, w, h = _regions_view(ref, (iw, ih), crop, size, filter)
        shape = (n, h, w) if m == capi.HM_REGIONS_STACK else (h, w)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device="cuda")
        elif not out.is_cuda or out.dtype != dtype:
            raise ValueError(f"out: a CUDA tensor of dtype {dtype} is needed, got {out.dtype} on {out.device}")
        elif tuple(out.shape) != shape:
            raise ValueError(f"out: shape {tuple(out.shape)} does not match the regions' {shape}")
        if out.numel() and out.stride(-1) != 1 and out.shape[-1] != 1:
            raise ValueError("out: the pixels of a row must be contiguous (only the row and plane strides are free)")
        es = out.element_size()
        d = capi.RegionsDest()
        d.ptr = out.data_ptr()
        d.len = out.untyped_storage().nbytes() - out.storage_offset() * es
        d.dtype = code
        d.row_pitch = out.stride(-2) * es
        d.plane_pitch = out.stride(0) * es if m == capi.HM_REGIONS_STACK and n > 1 else 0
        d.scale, d.bias = 1.0 if scale is None else float(scale), 0.0 if bias is None else float(bias)
        arr = (C.c_uint32 * len(ids))(*ids)
        res = capi.RegionsOut()
        with torch.cuda.device(out.device):
            (stream if hasattr(stream, "synchronize") else torch.cuda.current_stream(out.device)).synchronize()
            capi.check_image(L.hm_regions_to_device(f.h, arr, len(ids), C.byref(view) if view is not None else None, m, C.byref(d), C.byref(res)))
        if (res.width, res.height) != (w, h):
            raise capi.HmError(-6, f"the planes written are {res.width} x {res.height}, {w} x {h} were expected")
        return out
    finally:
        f.close()
