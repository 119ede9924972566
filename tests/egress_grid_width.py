"""Child process of tests/test_gpu_egress_regimes.py test_the_push_with_another_grid_width: KICP_PRE_PUSH_WGS is read once per
process, so every other width than the default needs a process of its own.  Runs the exact-boundary and the all-eight-full cases
through Frame and FrameF32 under the width the environment sets - under 0 (the DMA engine moves the doubles, queued behind
chain.ready; records are still pushed) also a frame of 1 MiB and more (three transfers, an event behind each) and a small one (one
event) -, prints one line per case and exits non-zero at the first mismatch; nothing is started after it."""
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]


def main():
    import egress_cases as ec
    import kinematic_icp_amd as K
    import test_gpu_egress_regimes as R
    wgs = int(os.environ["KICP_PRE_PUSH_WGS"])
    runs = [(case, f32) for case in ec.EXACT_BOUNDARY + ec.ALL_FULL for f32 in (False, True)]
    if wgs <= 0:
        runs += [(ec.DMA_PIECES, False), (ec.DMA_ONE_EVENT, False)]
    for case, f32 in runs:
        pushed = f32 or wgs > 0
        try:  # (the DMA engine moves room for every input point: only the frame itself is promised then, not what lies behind it)
            R.check_push(K.PreSteps(), case, f32, pushed=pushed, sentinel=pushed)
        except Exception:
            traceback.print_exc()
            print("MISMATCH %s %s wgs=%d" % (case, "FrameF32" if f32 else "Frame", wgs))
            return 1
        print("ok %s %s wgs=%d %s" % (case, "FrameF32" if f32 else "Frame", wgs, "pushed" if pushed else "dma"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
