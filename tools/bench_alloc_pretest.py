"""bench.py with the alloc walk's pre-test counters of its timed region: bench.py resets the scene's counters
where the timed region starts (Recon.reset_stats) and reads them where it ends (Recon.scene_stats); this wrapper
prints bf_recon_alloc_pretest_stats at that read, as one ALLOC_PRETEST line on stderr, and changes nothing else.
Usage: python3 tools/bench_alloc_pretest.py [bench.py's arguments]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bundlefusion_amd.recon as recon  # noqa: E402

_scene_stats = recon.Recon.scene_stats


def scene_stats(self):
    ss = _scene_stats(self)
    print("ALLOC_PRETEST " + json.dumps({"pretest": self.alloc_pretest_stats(), "integrateOps": ss["integrateOps"],
                                          "candidates": ss["candidates"], "allocated": ss["allocated"]}),
          file=sys.stderr, flush=True)
    return ss


recon.Recon.scene_stats = scene_stats
import bench  # noqa: E402

bench.main()
