#!/usr/bin/env python3
"""The unpack of ISO/IEC 23001-17 uncompressed items (hm_unci_unpack, csrc/unci.hip), timed on the GPU box from the repo root:

    python3 tools/bench_device_unci.py --out profiles/device_unci.txt

Three synthetic 8192 x 8192 items of random bytes in device memory (every bit pattern is a valid sample):
    8-bit R G B, pixel interleave, 256 x 256 internal tiles   -> R, G, B planes, and -> interleaved RGB24 (the byte path)
    8-bit 4:2:0, component interleave                          -> Y, Cb, Cr planes (the byte path: runs of 4 bytes)
    5-6-5 R G B, pixel interleave                               -> R, G, B planes (the generic path: two dwords and a funnel shift per sample)
Each launch is timed with device events, REPEATS times behind WARM warm-up launches, alternating with a device-to-device copy that
moves the same number of bytes (a copy of n bytes reads n and writes n: n = (bytes read + bytes written) / 2 of the unpack).  The rate
of a launch is (payload bytes read + output bytes written) / time; the ratio is copy time / unpack time.  Nothing here is a pass /
fail check."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 8192
REPEATS, WARM = 20, 3
RGB = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=W, help="width and height (a multiple of 256)")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    w = h = args.size

    def info(components, interleave, sampling=0, tile=None):
        u = capi.UnciInfo()
        u.width, u.height, u.n_components = w, h, len(components)
        types = {t for t, _ in components}
        u.colour_space = capi.HM_UNCI_YCBCR if capi.HM_UNCI_TYPE_Y in types else capi.HM_UNCI_RGB
        for c, (t, d) in enumerate(components):
            u.comp[c].type, u.comp[c].depth, u.comp[c].align_size = t, d, 0
        u.sampling, u.interleave = sampling, interleave
        u.tile_width, u.tile_height = tile or (w, h)
        u.tile_cols, u.tile_rows = w // u.tile_width, h // u.tile_height
        n = C.c_uint64()
        capi.check_image(L.hm_unci_payload_bytes(C.byref(u), C.byref(n)))
        u.payload_bytes = n.value
        return u

    R, G, B, Y, CB, CR = (capi.HM_UNCI_TYPE_R, capi.HM_UNCI_TYPE_G, capi.HM_UNCI_TYPE_B, capi.HM_UNCI_TYPE_Y, capi.HM_UNCI_TYPE_CB, capi.HM_UNCI_TYPE_CR)
    rgb8 = info([(R, 8), (G, 8), (B, 8)], capi.HM_UNCI_INTERLEAVE_PIXEL, tile=(256, 256))
    yuv420 = info([(Y, 8), (CB, 8), (CR, 8)], capi.HM_UNCI_INTERLEAVE_COMPONENT, capi.HM_UNCI_SAMPLING_420)
    rgb565 = info([(R, 5), (G, 6), (B, 5)], capi.HM_UNCI_INTERLEAVE_PIXEL)
    stride = capi.lib().hm_plane_stride(w, 1)
    print("payload bytes:", ", ".join(str(int(u.payload_bytes)) for u in (rgb8, yuv420, rgb565)))
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    plane_mem = [torch.empty((h, stride), dtype=torch.uint8, device="cuda") for _ in range(3)]
    pixels = torch.empty((h, w * 3), dtype=torch.uint8, device="cuda")

    def planes_of(u):
        p = capi.Planes()
        for c in range(3):
            p.plane[c], p.stride[c] = plane_mem[c].data_ptr(), stride
        return p

    dest = capi.DeviceDest(pixels.data_ptr(), pixels.numel(), capi.HM_DEV_LAYOUT_HWC, capi.HM_DEV_U8, w * 3, 0)
    cases = []
    for label, u, to_pixels, written in (("8-bit RGB, pixel mode, 256 x 256 tiles -> planes", rgb8, False, 3 * w * h),
                                         ("8-bit RGB, pixel mode, 256 x 256 tiles -> RGB24", rgb8, True, 3 * w * h),
                                         ("8-bit 4:2:0, component mode -> planes", yuv420, False, w * h * 3 // 2),
                                         ("5-6-5, pixel mode -> planes", rgb565, False, 3 * w * h)):
        payload = torch.randint(0, 256, (int(u.payload_bytes),), dtype=torch.uint8, device="cuda", generator=gen)
        moved = int(u.payload_bytes) + written
        a = torch.empty((moved // 2,), dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        p = planes_of(u)

        def unpack(u=u, payload=payload, p=p, to_pixels=to_pixels):
            capi.check_image(L.hm_unci_unpack(C.byref(u), payload.data_ptr(), payload.numel(), None, None if to_pixels else C.byref(p), RGB if to_pixels else 0,
                                              C.byref(dest) if to_pixels else None, st))
        cases.append((label, moved, unpack, lambda a=a, b=b: b.copy_(a)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"device: {torch.cuda.get_device_name(0)}; {w} x {h} items of random bytes in device memory; device events around one launch, {REPEATS} repeats behind {WARM} warm-up "
             "launches, unpack and copy alternating; ms: median (min .. max); GB/s = (bytes read + bytes written) / median",
             "the copy: a device-to-device copy of (bytes read + bytes written) / 2 bytes; ratio = copy time / unpack time (1.00: as fast as the copy)"]
    for label, moved, unpack, copy in cases:
        for _ in range(WARM):
            unpack()
            copy()
        torch.cuda.synchronize()
        tu, tc = [], []
        for _ in range(REPEATS):
            tu.append(timed(unpack))
            tc.append(timed(copy))
        mu, mc = statistics.median(tu), statistics.median(tc)
        lines.append(f"{label:52s} unpack {mu:7.3f} ({min(tu):.3f} .. {max(tu):.3f}) ms {moved / mu / 1e6:7.0f} GB/s | copy {mc:7.3f} ({min(tc):.3f} .. {max(tc):.3f}) ms "
                     f"{moved / mc / 1e6:7.0f} GB/s | ratio {mc / mu:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
