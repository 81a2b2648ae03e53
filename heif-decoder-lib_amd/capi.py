"""ctypes bindings of include/heif_mi355x.h.  No CPU fallback: if the shared library
is missing, loading raises; if there is no GPU the device entry points return
HM_ERR_NO_DEVICE and HmError is raised."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libheif_mi355x.so")
# the same objects + csrc/test_hooks.cpp (hm_debug_set, hm_debug_kernel_regs): tests and measurement scripts that force a cut of the
# chain kernel, inject a fault or read a kernel's registers load THIS one (use_test_hooks() before the first lib()); the shipping
# library exports no such entry point
TEST_LIB_PATH = os.path.join(_HERE, "libheif_mi355x_test.so")

HM_CHROMA_420, HM_CHROMA_422, HM_CHROMA_444 = 1, 2, 3
HM_OUT_RGB, HM_OUT_RGBA, HM_OUT_RRGGBB_BE, HM_OUT_RRGGBB_LE = 10, 11, 12, 14
HM_OUT_RRGGBBAA_BE, HM_OUT_RRGGBBAA_LE = 13, 15
HM_PIPE_INT420, HM_PIPE_FLOAT, HM_PIPE_BILINEAR_FLOAT, HM_PIPE_TO_HDR_FLOAT, HM_PIPE_MONO = 1, 2, 3, 4, 5
HM_PIPE_SDR_INT420, HM_PIPE_FLOAT_SDR, HM_PIPE_FLOAT_HDR = 6, 7, 8
HM_PIPE_PLANAR = 10
# planar YCbCr targets; HM_OUT_YCBCR_8BIT: or-ed where no convert_hdr_to_8bit field exists (ColourDesc, pipeline config)
HM_OUT_YCBCR_420, HM_OUT_YCBCR_422, HM_OUT_YCBCR_444, HM_OUT_YCBCR_8BIT = 0x101, 0x102, 0x103, 0x200
HM_PLANAR_UNFUSED = 1
# device-resident output (hm_device_dest)
HM_DEV_LAYOUT_HWC, HM_DEV_LAYOUT_CHW = 0, 1
HM_DEV_U8, HM_DEV_U16, HM_DEV_F16, HM_DEV_F32 = 0, 1, 2, 3
# device-resident planar YCbCr (hm_device_planes)
HM_DEV_PLANES_SEPARATE, HM_DEV_PLANES_SEMI = 0, 1
# views (hm_device_view): a rectangle of the image at a size of the caller's choice
HM_VIEW_TRIANGLE, HM_VIEW_NEAREST = 0, 1
HM_VIEW_CUBIC, HM_VIEW_LANCZOS3 = 16, 17
HM_VIEWS_MOST = 4096  # views of one hm_decode_item_to_device_views / hm_resample_views_to_tensor call
HM_PIPELINE_FULL = 1
HM_DETAIL_NO_COLOUR_CHAIN = 2


class HmError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__(f"heif_mi355x status {status}: {detail}")
        self.status = status


class ColourDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "bit_depth", "chroma", "has_nclx", "matrix", "primaries",
        "full_range", "out_format", "y_stride", "cb_stride", "cr_stride", "out_stride", "chroma_upsampling", "has_alpha")]


class Planes(C.Structure):
    """hm_planes: Y, Cb, Cr, alpha device pointers and their strides in bytes"""
    _fields_ = [("plane", C.c_void_p * 4), ("stride", C.c_int32 * 4)]


_lib = None


def use_test_hooks():
    """Make lib() load libheif_mi355x_test.so (test infrastructure: tests/knobs.py, tools/).  Must come before the first lib()."""
    global LIB_PATH
    if _lib is not None and LIB_PATH != TEST_LIB_PATH:
        raise RuntimeError("the shipping library is already loaded in this process: call use_test_hooks() first")
    LIB_PATH = TEST_LIB_PATH


def lib():
    """Load libheif_mi355x.so (built in-tree by __graft_entry__.build()); fail loudly if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} not built - run `python -c 'import __graft_entry__ as g; g.build()'`")
        # torch ships its own libamdhip64; it must be the one HIP runtime of the process, so
        # load it before our library binds libamdhip64 (two runtimes => "no ROCm-capable device")
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.hm_status_string.restype = C.c_char_p
        L.hm_last_error.restype = C.c_char_p
        L.hm_version.restype = C.c_char_p
        L.hm_colour_convert.argtypes = [C.POINTER(ColourDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hm_colour_pipeline.argtypes = [C.POINTER(ColourDesc)]
        L.hm_colour_convert_planar.argtypes = [C.POINTER(ColourDesc), C.POINTER(Planes), C.c_int, C.POINTER(Planes), C.c_int, C.c_void_p]
        L.hm_ycbcr_coefficients.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        bind_decode(L)
        _lib = L
    return _lib


def check(status):
    if status < 0:
        L = lib()
        raise HmError(status, f"{L.hm_status_string(status).decode()}: {L.hm_last_error().decode()}")
    return status


class TileDest(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("canvas_width", C.c_int32), ("canvas_height", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32),
                ("tile_has_nclx", C.c_int32), ("tile_full_range", C.c_int32), ("tile_matrix", C.c_int32)]


def bind_decode(L):
    """argtypes of the parse / batch entry points (called once from lib())."""
    L.hm_hevc_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.hm_free.argtypes = [C.c_void_p]
    L.hm_batch_create.argtypes = [C.POINTER(C.c_void_p)]
    L.hm_batch_destroy.argtypes = [C.c_void_p]
    L.hm_batch_clear.argtypes = [C.c_void_p]
    L.hm_batch_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(TileDest)]
    L.hm_batch_size.argtypes = [C.c_void_p]
    L.hm_batch_upload.argtypes = [C.c_void_p, C.c_void_p]
    L.hm_batch_execute.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.hm_batch_upload_execute.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hm_batch_tail_fused.argtypes = [C.c_void_p]
    L.hm_batch_tail_fused.restype = C.c_int
    L.hm_batch_set_colour.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.hm_batch_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.hm_batch_set_concurrency.argtypes = [C.c_void_p, C.c_int]
    L.hm_batch_get_timings.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.hm_batch_get_timings4.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.hm_batch_get_timings5.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.hm_batch_algorithmic_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]


class ImageInfo(C.Structure):
    """hm_image_info"""
    _fields_ = [(n, C.c_int32) for n in "width height bit_depth chroma is_grid grid_rows grid_cols tile_width tile_height has_transforms has_alpha coded_width coded_height has_nclx".split()]


class DecodeParams(C.Structure):
    """hm_decode_params"""
    _fields_ = [("out_format", C.c_int32), ("host_threads", C.c_int32), ("ignore_transformations", C.c_int32),
                ("chroma_upsampling", C.c_int32), ("stream", C.c_void_p), ("ext_dst", C.c_void_p),
                ("ext_dst_len", C.c_uint32), ("ext_dst_stride", C.c_uint32), ("strict_decoding", C.c_int32),
                ("convert_hdr_to_8bit", C.c_int32)]


class Decoded(C.Structure):
    """hm_decoded"""
    _fields_ = [(n, C.c_int32) for n in "width height bit_depth chroma out_format has_nclx primaries transfer matrix full_range used_ext_dst".split()] + \
               [("plane", C.POINTER(C.c_uint8) * 3), ("stride", C.c_int32 * 3), ("plane_width", C.c_int32 * 3), ("plane_height", C.c_int32 * 3),
                ("has_alpha", C.c_int32), ("alpha", C.POINTER(C.c_uint8)), ("alpha_stride", C.c_int32), ("warnings", C.c_int32)]


class DeviceDest(C.Structure):
    """hm_device_dest: caller-owned device memory the pixels of a decode go to"""
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_uint64), ("layout", C.c_int32), ("dtype", C.c_int32),
                ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class DevicePlane(C.Structure):
    """hm_device_plane: one plane of an hm_device_planes"""
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_uint64), ("row_pitch", C.c_int64)]


class DevicePlanes(C.Structure):
    """hm_device_planes: caller-owned device memory the planes of a planar YCbCr decode go to (Y, Cb | CbCr, Cr, alpha)"""
    _fields_ = [("plane", DevicePlane * 4), ("layout", C.c_int32), ("dtype", C.c_int32), ("msb_aligned", C.c_int32), ("reserved", C.c_int32),
                ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class DeviceView(C.Structure):
    """hm_device_view: crop rectangle (0, 0, 0, 0 = the whole image), output size (0, 0 = the crop's own), filter"""
    _fields_ = [(n, C.c_int32) for n in "crop_x crop_y crop_w crop_h out_w out_h filter".split()]


class DeviceLight(C.Structure):
    """hm_device_light: H.273 codes of the source (0 = the image's own) and of the result (to_transfer 8 = linear light, to_primaries
    0 = the source's), the gain on linear light"""
    _fields_ = [("from_transfer", C.c_int32), ("from_primaries", C.c_int32), ("to_transfer", C.c_int32), ("to_primaries", C.c_int32), ("gain", C.c_float),
                ("reserved", C.c_int32 * 3)]


HM_LIGHT_LINEAR = 8
HM_LIGHT_FROM_ICC = -1  # in from_transfer AND from_primaries: the item's ICC profile is the source
HM_ICC_RGB, HM_ICC_GRAY = 1, 2
HM_ICC_CURVE_IDENTITY, HM_ICC_CURVE_GAMMA, HM_ICC_CURVE_TABLE, HM_ICC_CURVE_PARA = 0, 1, 2, 3
HM_ICC_NO_PROFILE = 1   # hm_file_item_icc_info: the item has none


class IccCurve(C.Structure):
    """hm_icc_curve: kind (HM_ICC_CURVE_*), count ('curv': entries, 'para': function type), p = g a b c d e f"""
    _fields_ = [("kind", C.c_int32), ("count", C.c_int32), ("p", C.c_double * 7)]


class IccInfo(C.Structure):
    """hm_icc_info: what hm_icc_parse reports of a matrix/TRC profile"""
    _fields_ = [("version_major", C.c_int32), ("version_minor", C.c_int32), ("colour_space", C.c_int32), ("same_curves", C.c_int32), ("has_cicp", C.c_int32),
                ("cicp", C.c_int32 * 4), ("cicp_known", C.c_int32), ("colorant", C.c_double * 9), ("curve", IccCurve * 3)]


class DeviceTone(C.Structure):
    """hm_device_tone: the BT.2390 curve inside a light step - peaks and units in cd/m2 (src_peak 0 = the image's own, unit_nits 0 =
    10000 for PQ, out_unit_nits 0 = dst_peak), out_bits 8 = the 8-bit finish"""
    _fields_ = [("curve", C.c_int32), ("out_bits", C.c_int32), ("src_peak", C.c_float), ("dst_peak", C.c_float), ("unit_nits", C.c_float),
                ("out_unit_nits", C.c_float), ("reserved", C.c_int32 * 2)]


HM_TONE_BT2390 = 1
HM_TONE_STEPS = 2048


class DeviceAlpha(C.Structure):
    """hm_device_alpha: the mode, and for HM_ALPHA_MATTE the background's R, G, B code values at the target's sample depth"""
    _fields_ = [("mode", C.c_int32), ("background", C.c_uint16 * 4), ("reserved", C.c_int32 * 3)]


HM_ALPHA_STRAIGHT, HM_ALPHA_PREMULTIPLIED, HM_ALPHA_MATTE = 1, 2, 3


class GainParams(C.Structure):
    """hm_gain_params: the parameters of a gain map (ISO 21496-1) - headrooms, min and max are log2 values, per colour channel R, G, B"""
    _fields_ = [("base_headroom", C.c_double), ("alternate_headroom", C.c_double), ("map_min", C.c_double * 3), ("map_max", C.c_double * 3),
                ("gamma", C.c_double * 3), ("base_offset", C.c_double * 3), ("alternate_offset", C.c_double * 3), ("use_base_primaries", C.c_int32),
                ("reserved", C.c_int32)]


class GainMapInfo(C.Structure):
    """hm_gain_map_info: a 'tmap' item's base image, gain-map image, parameters and the alternate rendition's nclx profile"""
    _fields_ = [("base_item", C.c_uint32), ("map_item", C.c_uint32), ("params", GainParams), ("alt_has_nclx", C.c_int32), ("alt_primaries", C.c_int32),
                ("alt_transfer", C.c_int32)]


class DeviceGain(C.Structure):
    """hm_device_gain: the gain step beside a light step - map_item 0: the decoded item is a 'tmap' item; else the item of the map, with
    explicit params; headroom = log2(display peak / SDR white)"""
    _fields_ = [("map_item", C.c_uint32), ("headroom", C.c_float), ("params", GainParams), ("reserved", C.c_int32 * 4)]


class DeviceOotf(C.Structure):
    """hm_device_ootf: the HLG OOTF beside a light step - display_peak in cd/m2, gamma 0 = the system gamma of that peak"""
    _fields_ = [("kind", C.c_int32), ("display_peak", C.c_float), ("gamma", C.c_float), ("reserved", C.c_int32 * 5)]


HM_OOTF_HLG = 1
HM_OOTF_STEPS = 1024
HM_LIGHT_STATS_BINS = 2048


class LightStatsC(C.Structure):
    """hm_light_stats: the light statistics of a rectangle of pixels - the histogram over the tone step's 11-bit PQ codes of the pixels'
    norms, the largest norm, and what the host reads off them"""
    _fields_ = [("pixels", C.c_uint64), ("hist", C.c_uint32 * HM_LIGHT_STATS_BINS), ("max_norm", C.c_float), ("max_code", C.c_int32),
                ("max_nits", C.c_float), ("average_nits", C.c_float), ("reserved", C.c_int32 * 2)]


class LightLevels(C.Structure):
    """hm_light_levels: the raw fields of an item's clli and mdcv properties"""
    _fields_ = [("has_clli", C.c_int32), ("has_mdcv", C.c_int32), ("max_content_light_level", C.c_uint16), ("max_pic_average_light_level", C.c_uint16),
                ("display_primaries_x", C.c_uint16 * 3), ("display_primaries_y", C.c_uint16 * 3), ("white_point_x", C.c_uint16), ("white_point_y", C.c_uint16),
                ("max_display_mastering_luminance", C.c_uint32), ("min_display_mastering_luminance", C.c_uint32)]


class OverlayInfo(C.Structure):
    """hm_overlay_info"""
    _fields_ = [("canvas_width", C.c_int32), ("canvas_height", C.c_int32), ("n_children", C.c_int32), ("background", C.c_uint16 * 4)]


HM_ITEM_OTHER, HM_ITEM_HVC1, HM_ITEM_GRID, HM_ITEM_IDEN, HM_ITEM_IOVL, HM_ITEM_TMAP = 0, 1, 2, 3, 4, 5
HM_ITEM_UNCI = 6
HM_ITEM_MSKI = 7

# regions and masks ('rgan' / 'mski'): hm_region, hm_regions_dest
HM_REGION_POINT, HM_REGION_RECTANGLE, HM_REGION_ELLIPSE, HM_REGION_POLYGON, HM_REGION_REFERENCED_MASK, HM_REGION_INLINE_MASK, HM_REGION_POLYLINE = range(7)
REGION_TYPE_NAMES = ("point", "rectangle", "ellipse", "polygon", "referenced_mask", "inline_mask", "polyline")
HM_REGIONS_STACK, HM_REGIONS_LABELS = 0, 1


class RegionItemInfo(C.Structure):
    """hm_region_item_info"""
    _fields_ = [("reference_width", C.c_uint32), ("reference_height", C.c_uint32), ("n_regions", C.c_int32), ("field_bits", C.c_int32)]


class Region(C.Structure):
    """hm_region: x, y, w, h are centre and radii for an ellipse"""
    _fields_ = [("type", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_uint32), ("h", C.c_uint32), ("n_points", C.c_uint32),
                ("mask_item", C.c_uint32), ("mask_bytes", C.c_uint64)]


class RegionsDest(C.Structure):
    """hm_regions_dest: caller-owned device memory the planes of a region raster go to"""
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_uint64), ("dtype", C.c_int32), ("reserved", C.c_int32), ("row_pitch", C.c_int64),
                ("plane_pitch", C.c_int64), ("scale", C.c_float), ("bias", C.c_float)]


class RegionsOut(C.Structure):
    """hm_regions_out"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_regions", C.c_int32), ("planes", C.c_int32), ("bytes", C.c_int64),
                ("reference_width", C.c_uint32), ("reference_height", C.c_uint32)]


# uncompressed items (ISO/IEC 23001-17): hm_unci_info
HM_UNCI_MONO, HM_UNCI_YCBCR, HM_UNCI_RGB = 0, 1, 2
HM_UNCI_MAX_COMPONENTS = 8
HM_UNCI_TYPE_MONO, HM_UNCI_TYPE_Y, HM_UNCI_TYPE_CB, HM_UNCI_TYPE_CR, HM_UNCI_TYPE_R, HM_UNCI_TYPE_G, HM_UNCI_TYPE_B, HM_UNCI_TYPE_ALPHA = range(8)
HM_UNCI_TYPE_PADDED = 12
HM_UNCI_INTERLEAVE_COMPONENT, HM_UNCI_INTERLEAVE_PIXEL, HM_UNCI_INTERLEAVE_MIXED, HM_UNCI_INTERLEAVE_ROW, HM_UNCI_INTERLEAVE_TILE_COMPONENT = range(5)
HM_UNCI_SAMPLING_NONE, HM_UNCI_SAMPLING_422, HM_UNCI_SAMPLING_420 = 0, 1, 2


class UnciComponent(C.Structure):
    """hm_unci_component"""
    _fields_ = [("type", C.c_uint16), ("depth", C.c_uint8), ("align_size", C.c_uint8)]


class UnciInfo(C.Structure):
    """hm_unci_info: what the cmpd and uncC properties of an 'unci' item say, and the byte length its layout needs"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("colour_space", C.c_int32), ("n_components", C.c_int32),
                ("comp", UnciComponent * HM_UNCI_MAX_COMPONENTS), ("sampling", C.c_int32), ("interleave", C.c_int32),
                ("pixel_size", C.c_uint32), ("row_align", C.c_uint32), ("tile_align", C.c_uint32),
                ("tile_cols", C.c_uint32), ("tile_rows", C.c_uint32), ("tile_width", C.c_uint32), ("tile_height", C.c_uint32),
                ("payload_bytes", C.c_uint64)]


class SequenceInfo(C.Structure):
    """hm_sequence_info"""
    _fields_ = [("is_sequence", C.c_int32), ("frame_count", C.c_uint32), ("duration", C.c_uint64)]


class PipelineConfig(C.Structure):
    """hm_pipeline_config"""
    _fields_ = [(n, C.c_int32) for n in "host_threads max_in_flight out_format chroma_upsampling ignore_transformations strict_decoding device cpu_first cpu_count".split()]


class PipelineResult(C.Structure):
    """hm_pipeline_result"""
    _fields_ = [("tag", C.c_uint64), ("status", C.c_int32), ("image", Decoded), ("handle", C.c_void_p)]


# ---- the device entries of the item, frames and pipeline families: one table behind their argtypes (bind_image) and behind the choice of
#      the entry a request goes through (entry_of; decode.py) ----
STEP_TYPES = {"view": DeviceView, "light": DeviceLight, "tone": DeviceTone, "alpha": DeviceAlpha, "gain": DeviceGain, "ootf": DeviceOotf}
# the kinds, in the precedence a request picks its entry by: the suffix of the entry's name, the step that picks it, its step arguments in order
ENTRY_KINDS = (("_gain", "gain", ("view", "light", "tone", "gain")),
               ("_ootf", "ootf", ("view", "light", "ootf", "tone", "alpha")),
               ("_alpha", "alpha", ("view", "light", "tone", "alpha")),
               ("_tone", "tone", ("view", "light", "tone")),
               ("_light", "light", ("view", "light")),
               ("_view", "view", ("view",)),
               ("", None, ()))
PLANES_KINDS = (("_planes_view", "view", ("view",)), ("_planes", None, ()))
_FRAMES_TAIL = [C.POINTER(Decoded), C.POINTER(C.c_int32)]
# family -> argtypes before the steps, behind them (interleaved, planar), the kinds it lacks, the steps none of its entries takes.
# The last kind a family has is the entry of a request that picks none: the frames family has no plain entry, its _view entry takes a
# null view.
ENTRY_FAMILIES = {
    "hm_decode_item_to_device": ([C.c_void_p, C.c_uint32, C.POINTER(DecodeParams)], [C.POINTER(DeviceDest), C.POINTER(Decoded)],
                                 [C.POINTER(DevicePlanes), C.POINTER(Decoded)], (), ()),
    "hm_decode_frames_to_device": ([C.c_void_p, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(DecodeParams)], [C.POINTER(DeviceDest)] + _FRAMES_TAIL,
                                   [C.POINTER(DevicePlanes)] + _FRAMES_TAIL, ("_gain", "_alpha", ""), ("alpha", "gain")),
    "hm_pipeline_submit_to_device": ([C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint64], [C.POINTER(DeviceDest)], [C.POINTER(DevicePlanes)], (), ()),
}


def entry_of(family, given, planes=False):
    """(name of the entry of `family` that a request holding the steps `given` - names of STEP_TYPES - goes through, the names of that
    entry's step arguments in order); planes: the family's entries for planar destinations"""
    _, _, _, lacks, no_steps = ENTRY_FAMILIES[family]
    kinds = [k for k in (PLANES_KINDS if planes else ENTRY_KINDS) if k[0] not in lacks or planes]
    suffix, _, steps = next((k for k in kinds if k[1] in given), kinds[-1])
    return family + suffix, [s for s in steps if s not in no_steps]


_image_lib = None


def image_lib():
    """The library once more, as a ctypes object of its own with the image-level entry points bound to the structures above (the
    same loaded library as lib(): ctypes keeps argtypes per object, and callers of lib() bind these entry points to structure
    classes of their own)."""
    global _image_lib
    if _image_lib is None:
        lib()
        L = C.CDLL(LIB_PATH)
        L.hm_status_string.restype = C.c_char_p
        L.hm_last_error.restype = C.c_char_p
        bind_image(L)
        _image_lib = L
    return _image_lib


def check_image(status):
    if status < 0:
        L = image_lib()
        raise HmError(status, f"{L.hm_status_string(status).decode()}: {L.hm_last_error().decode()}")
    return status


def bind_image(L):
    """argtypes of the file / image / sequence / pipeline entry points and of the device-destination ones."""
    L.hm_file_open.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.hm_file_close.argtypes = [C.c_void_p]
    L.hm_file_close.restype = None
    L.hm_file_primary_item.argtypes = [C.c_void_p]
    L.hm_file_primary_item.restype = C.c_uint32
    L.hm_file_image_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ImageInfo)]
    L.hm_file_sequence_info.argtypes = [C.c_void_p, C.POINTER(SequenceInfo)]
    L.hm_file_top_level_images.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    L.hm_file_item_kind.argtypes = [C.c_void_p, C.c_uint32]
    L.hm_file_overlay_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(OverlayInfo), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_int]
    L.hm_file_derived_child.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.hm_plan_overlay.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.POINTER(C.c_int32), C.c_int]
    L.hm_decode_item.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(Decoded)]
    L.hm_decoded_free.argtypes = [C.POINTER(Decoded)]
    L.hm_decoded_free.restype = None
    L.hm_device_dest_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(DeviceDest)]
    L.hm_device_dest_bytes.restype = C.c_int64
    for family, (head, tail, planes_tail, lacks, no_steps) in ENTRY_FAMILIES.items():
        for kinds, behind in ((ENTRY_KINDS, tail), (PLANES_KINDS, planes_tail)):
            for suffix, _, steps in kinds:
                if suffix not in lacks:  # (every other name must be exported: a missing one fails here, by name)
                    getattr(L, family + suffix).argtypes = head + [C.POINTER(STEP_TYPES[s]) for s in steps if s not in no_steps] + behind
    L.hm_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceDest), C.c_void_p]
    L.hm_decode_sequence_to_device.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(DecodeParams), C.POINTER(DeviceDest),
                                               C.POINTER(Decoded), C.POINTER(C.c_int32)]
    L.hm_pipeline_create.argtypes = [C.POINTER(PipelineConfig), C.POINTER(C.c_void_p)]
    L.hm_pipeline_destroy.argtypes = [C.c_void_p]
    L.hm_pipeline_destroy.restype = None
    L.hm_pipeline_submit.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint64]
    L.hm_resample_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceDest), C.c_void_p]
    L.hm_plan_view.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.POINTER(C.c_int32 * 4)]
    L.hm_decode_item_to_device_views.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.POINTER(DeviceDest), C.c_int32,
                                                 C.POINTER(DeviceLight), C.POINTER(DeviceTone), C.POINTER(DeviceAlpha), C.POINTER(DeviceOotf), C.POINTER(Decoded),
                                                 C.POINTER(C.c_int32)]
    L.hm_resample_views_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceDest), C.c_int32, C.c_void_p]
    L.hm_plan_views.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.c_int32, C.POINTER(C.c_int32 * 4)]
    L.hm_view_filter_taps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int]
    L.hm_light_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceDest),
                                     C.c_void_p]
    L.hm_light_table.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_float)]
    L.hm_light_matrix.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float * 9)]
    L.hm_icc_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(IccInfo)]
    L.hm_icc_table.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float)]
    L.hm_icc_matrix.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_float * 9)]
    L.hm_file_item_icc_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(IccInfo)]
    L.hm_icc_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.c_char_p, C.c_size_t, C.POINTER(DeviceLight),
                                   C.POINTER(DeviceTone), C.POINTER(DeviceAlpha), C.POINTER(DeviceDest), C.c_void_p]
    L.hm_tone_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceTone),
                                    C.POINTER(DeviceDest), C.c_void_p]
    L.hm_tone_table.argtypes = [C.POINTER(DeviceTone), C.c_float, C.c_int, C.POINTER(C.c_float)]
    L.hm_file_item_light_levels.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(LightLevels)]
    L.hm_alpha_dest_format.argtypes = [C.c_int, C.POINTER(DeviceAlpha), C.POINTER(DeviceTone)]
    L.hm_alpha_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceTone),
                                     C.POINTER(DeviceAlpha), C.POINTER(DeviceDest), C.c_void_p]
    L.hm_file_gain_map_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(GainMapInfo)]
    L.hm_file_gain_map_of.argtypes = [C.c_void_p, C.c_uint32]
    L.hm_file_gain_map_of.restype = C.c_uint32
    L.hm_file_item_aux_type.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int]
    L.hm_gain_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DeviceView),
                                    C.POINTER(DeviceLight), C.POINTER(DeviceTone), C.POINTER(DeviceGain), C.POINTER(DeviceDest), C.c_void_p]
    L.hm_gain_table.argtypes = [C.POINTER(GainParams), C.c_float, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.hm_ootf_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceOotf),
                                    C.POINTER(DeviceTone), C.POINTER(DeviceAlpha), C.POINTER(DeviceDest), C.c_void_p]
    L.hm_ootf_gamma.argtypes = [C.POINTER(DeviceOotf), C.POINTER(C.c_double)]
    L.hm_ootf_table.argtypes = [C.POINTER(DeviceOotf), C.c_float, C.c_int, C.POINTER(C.c_float)]
    L.hm_ootf_luma.argtypes = [C.c_int, C.POINTER(C.c_float * 3)]
    L.hm_light_stats_code_nits.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.hm_light_stats_percentile.argtypes = [C.POINTER(LightStatsC), C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    L.hm_light_stats_average.argtypes = [C.POINTER(LightStatsC), C.POINTER(C.c_float)]
    L.hm_light_stats_of_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceOotf),
                                           C.c_float, C.POINTER(LightStatsC), C.c_void_p]
    L.hm_decode_item_light_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceOotf),
                                             C.c_float, C.POINTER(LightStatsC), C.POINTER(Decoded)]
    L.hm_decode_item_to_device_measured.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.POINTER(DeviceLight), C.POINTER(DeviceOotf),
                                                    C.POINTER(DeviceTone), C.c_double, C.POINTER(DeviceDest), C.POINTER(Decoded), C.POINTER(LightStatsC)]
    L.hm_device_planes_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DevicePlanes), C.POINTER(C.c_int64 * 4)]
    L.hm_device_planes_bytes.restype = C.c_int64
    L.hm_planes_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p * 4), C.POINTER(C.c_int32 * 4), C.POINTER(DevicePlanes),
                                      C.c_void_p]
    L.hm_planes_view_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(DeviceView), C.POINTER(C.c_int32 * 4 * 4), C.POINTER(C.c_int32 * 2 * 4)]
    L.hm_resample_planes_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p * 4), C.POINTER(C.c_int32 * 4),
                                               C.POINTER(DeviceView), C.POINTER(DevicePlanes), C.c_void_p]
    L.hm_plan_planes_view.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(DecodeParams), C.POINTER(DeviceView), C.POINTER(C.c_int32 * 4)]
    L.hm_file_unci_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(UnciInfo)]
    L.hm_unci_sample_bit.argtypes = [C.POINTER(UnciInfo), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.hm_unci_payload_bytes.argtypes = [C.POINTER(UnciInfo), C.POINTER(C.c_uint64)]
    L.hm_unci_unpack.argtypes = [C.POINTER(UnciInfo), C.c_void_p, C.c_size_t, C.POINTER(C.c_int32 * 4), C.POINTER(Planes), C.c_int, C.POINTER(DeviceDest),
                                 C.c_void_p]
    L.hm_file_region_items.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_int]
    L.hm_file_region_item_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RegionItemInfo)]
    L.hm_file_region.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Region)]
    L.hm_file_region_points.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_int32), C.c_int]
    L.hm_file_region_inline_mask.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.hm_regions_dest_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RegionsDest)]
    L.hm_regions_dest_bytes.restype = C.c_int64
    L.hm_rasterise_regions.argtypes = [C.POINTER(Region), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(DeviceView), C.c_int,
                                       C.POINTER(RegionsDest), C.c_void_p]
    L.hm_regions_to_device.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.POINTER(DeviceView), C.c_int, C.POINTER(RegionsDest),
                                       C.POINTER(RegionsOut)]
    L.hm_pipeline_pending.argtypes = [C.c_void_p]
    L.hm_pipeline_next.argtypes = [C.c_void_p, C.POINTER(PipelineResult)]
    L.hm_pipeline_release.argtypes = [C.c_void_p, C.POINTER(PipelineResult)]
    L.hm_pipeline_release.restype = None


class ParseOptions(C.Structure):
    """hm_parse_options (include/heif_mi355x.h)"""
    _fields_ = [("annexb", C.c_int32), ("threads", C.c_int32), ("record_order", C.c_int32)]


def parse_hevc(data, annexb=False, threads=1, record_order=None):
    """hm_hevc_parse[_mt] - or, with a record order (HM_RECORDS_*), hm_hevc_parse_opts - -> command-stream blob (bytes)."""
    L = lib()
    blob = C.POINTER(C.c_uint8)()
    size = C.c_size_t()
    L.hm_hevc_parse_mt.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hm_hevc_parse_mt.restype = C.c_int
    if record_order is not None:
        L.hm_hevc_parse_opts.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(ParseOptions), C.c_void_p, C.c_void_p]
        L.hm_hevc_parse_opts.restype = C.c_int
        o = ParseOptions(1 if annexb else 0, threads, record_order)
        check(L.hm_hevc_parse_opts(data, len(data), C.byref(o), C.byref(blob), C.byref(size)))
    elif threads > 1:
        check(L.hm_hevc_parse_mt(data, len(data), 1 if annexb else 0, threads, C.byref(blob), C.byref(size)))
    else:
        check(L.hm_hevc_parse(data, len(data), 1 if annexb else 0, C.byref(blob), C.byref(size)))
    out = C.string_at(blob, size.value)
    L.hm_free(blob)
    return out


def stream_header(blob):
    """(width, height, chroma_format, bit_depth, flags, full_range, matrix, primaries, has_vui_colour) of a command stream."""
    import struct
    magic, total, w, h = struct.unpack_from("<IIHH", blob, 0)
    cl, cr, ct, cb = struct.unpack_from("<4H", blob, 12)
    cf, bdy, bdc, l2ctb = struct.unpack_from("<BBBB", blob, 20)
    flags, = struct.unpack_from("<I", blob, 36)
    prim, trc, mat, fr = struct.unpack_from("<BBBB", blob, 40)
    return dict(width=w, height=h, crop=(cl, cr, ct, cb), chroma_format=cf, bit_depth=bdy, log2_ctb=l2ctb, flags=flags,
                primaries=prim, transfer=trc, matrix=mat, full_range=fr, has_vui_colour=bool(flags & 0x10))


class Batch:
    """Thin RAII wrapper of hm_batch."""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.hm_batch_create(C.byref(self.h)))

    def add(self, blob, dest):
        return check(self.L.hm_batch_add(self.h, blob, len(blob), C.byref(dest)))

    def upload(self, stream=None):
        check(self.L.hm_batch_upload(self.h, stream))

    def execute(self, stages=3, stream=None):
        check(self.L.hm_batch_execute(self.h, stages, stream))

    def upload_execute(self, stages, chunks, copy_stream, stream):
        check(self.L.hm_batch_upload_execute(self.h, stages, chunks, copy_stream, stream))

    def set_colour(self, desc, n_images, p_y, p_cb, p_cr, p_out, images_per_group=0):
        check(self.L.hm_batch_set_colour(self.h, C.byref(desc) if desc is not None else None, n_images, p_y, p_cb, p_cr, p_out, images_per_group))

    def clear(self):
        self.L.hm_batch_clear(self.h)

    def set_profiling(self, slots=1):
        check(self.L.hm_batch_set_profiling(self.h, int(slots)))

    def set_concurrency(self, groups):
        check(self.L.hm_batch_set_concurrency(self.h, int(groups)))

    def timings_ms(self, slot=0):
        ms = (C.c_float * 3)()
        check(self.L.hm_batch_get_timings(self.h, slot, ms))
        return [ms[0], ms[1], ms[2]]

    def timings4_ms(self, slot=0):
        ms = (C.c_float * 4)()
        check(self.L.hm_batch_get_timings4(self.h, slot, ms))
        return [ms[0], ms[1], ms[2], ms[3]]

    def timings5_ms(self, slot=0):
        """[chains (or the whole reconstruction), deblocking, SAO + paste (or the fused tail), colour, residual pre-pass]"""
        ms = (C.c_float * 5)()
        check(self.L.hm_batch_get_timings5(self.h, slot, ms))
        return [ms[i] for i in range(5)]

    def check(self):
        """waits for the batch; raises when a reconstruction wave gave up a bounded wait (hm_batch_check)"""
        self.L.hm_batch_check.argtypes = [C.c_void_p]
        check(self.L.hm_batch_check(self.h))

    def tail_fused(self):
        """True when the batch's executes run the fused tail kernel (timings4_ms: its time is in slot 2)"""
        return bool(self.L.hm_batch_tail_fused(self.h))

    def algorithmic_bytes4(self):
        """(command streams, reconstructed samples, levels, residual samples) in bytes"""
        v = (C.c_uint64 * 4)()
        self.L.hm_batch_algorithmic_bytes4.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        check(self.L.hm_batch_algorithmic_bytes4(self.h, v))
        return [int(x) for x in v]

    def algorithmic_bytes(self):
        a, b = C.c_uint64(), C.c_uint64()
        check(self.L.hm_batch_algorithmic_bytes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            self.L.hm_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def overlay_info(file_handle, item_id):
    """hm_file_overlay_info -> dict(canvas=(w, h), background=[r, g, b, a], layers=[(item id, dx, dy)]) of an 'iovl' item"""
    L = image_lib()
    info = OverlayInfo()
    check_image(L.hm_file_overlay_info(file_handle, item_id, C.byref(info), None, None, 0))
    n = info.n_children
    ids, offs = (C.c_uint32 * max(n, 1))(), (C.c_int32 * max(2 * n, 1))()
    check_image(L.hm_file_overlay_info(file_handle, item_id, C.byref(info), ids, offs, n))
    return dict(canvas=(info.canvas_width, info.canvas_height), background=list(info.background),
                layers=[(ids[i], offs[2 * i], offs[2 * i + 1]) for i in range(n)])


def derived_child(file_handle, item_id):
    """hm_file_derived_child: the image an 'iden' item derives from"""
    child = C.c_uint32()
    check_image(image_lib().hm_file_derived_child(file_handle, item_id, C.byref(child)))
    return child.value


def plan_overlay(file_handle, item_id, params, view=None):
    """hm_plan_overlay -> [True / False per layer]: which layers a decode (under `view`) decodes"""
    L = image_lib()
    n = check_image(L.hm_plan_overlay(file_handle, item_id, C.byref(params), C.byref(view) if view is not None else None, None, 0))
    dec = (C.c_int32 * max(n, 1))()
    check_image(L.hm_plan_overlay(file_handle, item_id, C.byref(params), C.byref(view) if view is not None else None, dec, n))
    return [bool(dec[i]) for i in range(n)]
