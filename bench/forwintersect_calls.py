"""Twelve Handle.forwintersect calls on a synth scene at its true EO, for a kernel trace: k_forwintersect's own time beside
bench/time_intersect.py, which can only print the wall time of the call.
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fwd -- python bench/forwintersect_calls.py C3
and read k_forwintersect's row of OUT/fwd_kernel_stats.csv.
bench/forwintersect_calls.py [C3 | C4 ...]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbat_amd import _hip, synth

for name in sys.argv[1:] or ['C3']:
    s, truth = synth.make_scene(name)
    s.EO.val[:6], s.IO.val[:] = truth['EO'][:6], truth['IO']
    h = _hip.Handle(s)
    try:
        x = h.serialize()
        for i in range(12):
            h.forwintersect(x, s.OP.val)
    finally:
        h.close()
    print(name, 'done', flush=True)
