"""The frame path with both track sets in ONE LK launch (larvio_amd/csrc/fe_frame.hip: track_chain_merged, k_fe_lk_pipe<21> with two
LkSets), HIP against the oracle frame by frame with the comparison of tests/test_gpu_frontend_edge.py (ids, lifetimes, points,
descriptors, new corners and the feature message bit for bit).  The merged launch is selected by LVK_LK_MERGED=1, read once per process
(lvk_lk_choice, lvk_internal.h: built and kept, not the default), so the module re-runs itself in one fresh child process with the
switch set; the child runs every case on one context and writes what it saw to a file.  The shapes are the smallest that reach the merged
launch with both sets populated (old tracks and the new corners detected behind a publish): 120 track slots, the default 21-pixel window,
14 frames; 336 x 200 with pyramid_levels=4 builds four levels, which is the most the five-wavefront kernel takes (LK_PIPE_MAX_LEVELS) -
the level bound of the rule."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (width, height, pyramid_levels, texture seed)
CASES = {"320x240_levels2": (320, 240, 2, 8), "336x200_levels4": (336, 200, 4, 1)}


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """what a process started with LVK_LK_MERGED=1 saw in every case"""
    path = str(tmp_path_factory.mktemp("lk_merged") / "out.json")
    env = dict(os.environ, LVK_LK_MERGED="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=240)
    out = json.load(open(path)) if os.path.exists(path) else {}
    return p, out


@pytest.mark.parametrize("name", sorted(CASES))
def test_merged_launch_matches_oracle_frame_by_frame(child, name):
    p, out = child
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    r = out[name]
    print(name, r)
    assert r["error"] is None, r["error"]
    assert r["states"][-1] == 3 and r["n_msgs"] >= 5 and r["n_tracks"][-1] > 40


def _worker(path):
    """every case on one fresh context, in a process whose LVK_LK_MERGED was 1 before the library was loaded"""
    assert os.environ.get("LVK_LK_MERGED") == "1"
    import larvio_amd
    from tests.test_gpu_frontend_edge import _run, _cfg, _texture, _crops, _walk
    ctx = larvio_amd.Context()
    out, failed = {}, False
    for name, (w, h, levels, seed) in CASES.items():
        frames = _crops(_texture(seed, h + 120, w + 160), w, h, _walk(14))
        rec = {"error": None, "states": [], "n_tracks": [], "n_msgs": 0}
        try:
            states, n_tracks, n_msgs = _run(ctx, frames, _cfg(w, h, max_features_num=120, min_distance=12, pyramid_levels=levels))
            rec.update(states=[int(s) for s in states], n_tracks=[int(n) for n in n_tracks], n_msgs=int(n_msgs))
            assert states[-1] == 3 and n_msgs >= 5 and n_tracks[-1] > 40, (states, n_tracks, n_msgs)
        except AssertionError as e:
            rec["error"] = repr(e); failed = True
        out[name] = rec
        json.dump(out, open(path, "w"))
        if failed:
            break                                   # (a front-end that failed a comparison was not closed: nothing more on this context)
    if not failed:
        ctx.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from tests import test_gpu_lk_merged as me
    sys.exit(me._worker(sys.argv[1]))
