"""hyb_clip_aug_u8_transform against the float64 rule (tests/randaug_ref.py) on the source, rows, sizes and variants of tests/test_gpu_randaug.py: per
family the worst error / gate over sizes and variants.  Geometry and hue: gate = 4 max|x32 - x64| + 2^-20 T with x32 the rule restated in numpy
float32 (the yardstick is the reference's own, never the kernel's); pointwise programs and quantising steps: the gate program_gate() derives from
the factors.  Pixels at a deciding boundary or at the frame's edge are left out as in the tests, and their share is printed.

    python scripts/randaug_errors.py [--out profiles/randaug_errors.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaug_errors.txt"))
    args = ap.parse_args()
    import test_gpu_randaug as T
    lines = ["hyb_clip_aug_u8_transform against the float64 rule (scripts/randaug_errors.py): the 3 clips x 5 frames of 37 x 53 of tests/test_gpu_randaug.py,",
             "Tout = 3, sizes 24 x 24, 9 x 13, 64 x 64 and 8 x 8, variants rgb-imagenet, rgb-plain and grey.  Per family the worst error / gate, with the",
             "case it occurs in.  geometry, hue: gate = 4 max|x32 - x64| + 2^-20 T (x32: the rule in numpy float32 on the CPU; T = max(1, max 1/std));",
             "program, quantising: the gate derived from the factors (tests/test_gpu_randaug.py, program_gate).  'left out': the largest share of pixels",
             "within 2^-10 of a deciding boundary or of the frame's edge (cap 2 %)."]
    worst = {}

    def note(family, ratio, out, text):
        if family not in worst or ratio > worst[family][0]:
            worst[family] = (ratio, max(out, worst.get(family, (0, 0))[1]), text)
        else:
            worst[family] = (worst[family][0], max(out, worst[family][1]), worst[family][2])
    for size in T.SIZES:
        for (C, norm), vid in zip(T.VARIANTS, T.VIDS):
            where = f"{size[0]} x {size[1]} {vid}"
            for family, aug in T.geometry_cases(size).items():
                err, gate, yard, out = T.geometry_errors(size, C, norm, family, aug)
                note(family, err / gate, out, f"{where}: error {err:.3e}, gate {gate:.3e}, fp32 restatement {yard:.3e}")
            Tn = T._scale(norm, C)
            for name, (progs, photo) in T.AFFINE.items():
                aug = [T.aug_row(p) for p in progs]
                tol = max(T.program_gate(p, None if photo is None else photo[b], Tn) for b, p in enumerate(progs))
                want, near = T._ref(size, C, norm, aug, photo=photo)
                err = T._err(T._aug(size, C, norm, aug, photo=photo), want)
                note("program", err / tol, float(near.mean()), f"{name}, {where}: error {err:.3e}, gate {tol:.3e}")
            for name, progs in T.QUANTISING.items():
                aug = [T.aug_row(p) for p in progs]
                tol = max(T.program_gate(p, None, Tn) for p in progs)
                want, near = T._ref(size, C, norm, aug)
                err = T._err(T._aug(size, C, norm, aug), want, T._kept(near))
                note("quantising", err / tol, float(near.mean()), f"{name}, {where}: error {err:.3e}, gate {tol:.3e}")
    for family, (ratio, out, text) in worst.items():
        lines.append(f"  {family:<22} error / gate {ratio:.3f}   left out <= {100 * out:.2f} %   {text}" + ("   ABOVE ONE HALF" if ratio > 0.5 else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
