"""Prints every stand-alone-entry (tensor_*) request of tests/target_cases.py as one line of plain values for tools/asan/target_walk.cpp,
which makes the calls itself (tools/asan/run_target_walk.sh pipes one into the other; nothing sanitised is loaded here):
    family fmt bits w h stride | view: 0 or 7 ints | light: 0 or 5 | tone: 0 or 6 | alpha: 0 or 8 | layout dtype ptr len row_pitch plane_pitch | label"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import __graft_entry__ as g
    import target_cases as tc
    capi = g.load_package().capi
    L = capi.image_lib()

    def group(values):
        return " ".join([str(len(values))] + [v.hex() if isinstance(v, float) else str(v) for v in values])

    def line(family, fmt, bits, w, h, stride, view, light, tone, alpha, d):
        steps = [list(view[0]) + list(view[1]) + [view[2]] if view else [], list(light) if light else [], list(tone) if tone else [],
                 [alpha[0]] + list(alpha[1]) + list(alpha[2]) if alpha else []]
        dest = [d.layout, d.dtype, d.ptr or 0, d.len, d.row_pitch, d.plane_pitch]
        return " ".join([family, str(fmt), str(bits), str(w), str(h), str(stride)] + [group(s) for s in steps] + [str(v) for v in dest])

    for name, families, over in tc.CASES:
        for family in families:
            if tc.FAMILIES[family]["call"] == "tensor":
                print(tc.run(capi, L, None, family, over, tensor_call=line), "|", f"{name} | {family}")


if __name__ == "__main__":
    main()
