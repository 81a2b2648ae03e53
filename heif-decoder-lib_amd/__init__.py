"""heif-decoder-lib_amd — MI355X-native HEIC hot path (HEVC-intra tile reconstruction,
deblock, SAO, grid paste and fused YCbCr->RGB) behind the reference's plugin / C API.

The product is the C-ABI shared library ``libheif_mi355x.so`` (HIP kernels for gfx950 +
C++ host code, see ``include/heif_mi355x.h``).  This package is only the thin Python
harness used by tests and ``bench.py``: ctypes bindings, torch for device memory/streams, and
``decode_to_tensor`` / ``decode_batch_to_tensor`` (decode.py): HEIF bytes to a CUDA tensor without a host round trip,
and ``decode_to_planes`` / ``decode_batch_to_planes`` / ``decode_sequence_to_planes``: the same to planar YCbCr (I420, NV12, P010);
``read_regions`` / ``decode_regions_to_tensor``: a file's region annotations and masks, read and rasterised to mask tensors;
``decode_to_views`` / ``crops_of_regions``: many crops of one picture from one decode;
``measure_light`` / ``measure_light_of_tensor``: a picture's light levels measured on the device (``LightStats``).

The directory name contains hyphens, so import it with ``load_package()`` from
``__graft_entry__`` (module name ``heif_decoder_lib_amd``).
"""
from . import capi  # noqa: F401
from . import shard  # noqa: F401
from .capi import lib, HmError  # noqa: F401
from .decode import decode_to_tensor, decode_batch_to_tensor, decode_sequence_to_tensor  # noqa: F401
from .decode import decode_to_planes, decode_batch_to_planes, decode_sequence_to_planes  # noqa: F401
from .decode import read_regions, decode_regions_to_tensor  # noqa: F401
from .decode import decode_to_views, crops_of_regions  # noqa: F401
from .decode import measure_light, measure_light_of_tensor, LightStats  # noqa: F401
