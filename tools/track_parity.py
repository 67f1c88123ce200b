"""The tracker's restatement (tests/track_ref.py) in float32 against the same code in float64, on every case tests/test_gpu_track.py
compares with the kernel bit for bit: whether the two runs make the same matches (they must: tests/test_track_ref.py asserts it),
and the largest difference between their posterior boxes, which is measured here and bounded nowhere.  Needs no device.

    python tools/track_parity.py [--out profiles/track_parity.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import track_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_parity.txt'))
    a = ap.parse_args()
    lines = ['float32 restatement against its float64 run (the thresholds, the constants and the rows are float32 values in both)',
             '%-22s %7s %7s %8s %9s %14s %14s' % ('case', 'streams', 'frames', 'matches', 'the same', 'max |d box| px', 'largest box px')]
    worst = 0.0
    for name, c in sorted(R.fixtures().items()):
        f32, f64 = R.run_case(c)[0], R.run_case(c, dtype=np.float64)[0]
        same = all(x[7] == y[7] and all(np.array_equal(x[k], y[k]) for k in (1, 2, 3, 4)) for x, y in zip(f32, f64))
        matches = sum(len(m) for x in f32 for m in x[7])
        d = big = 0.0
        for x, y in zip(f32, f64):
            for ba, bb in zip(x[6], y[6]):
                if len(ba):
                    d = max(d, float(np.abs(ba.astype(np.float64) - bb).max()))
                    big = max(big, float(np.abs(bb).max()))
        worst = max(worst, d)
        lines.append('%-22s %7d %7d %8d %9s %14.3e %14.1f' % (name, c['streams'], len(c['frames']), matches, 'yes' if same else 'NO', d, big))
    lines.append('largest difference of a posterior box coordinate over all cases: %.3e px' % worst)
    print('\n'.join(lines))
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
