"""Shadow replay of the corner detection under a caller-supplied region mask (lvk_frontend_set_mask).

The reference has no such mask, so the oracle's Frontend cannot be the judge of a masked run.  What can be: after every processed
frame, the detection is REPLAYED from the product's own live tracks with the oracle's existing stage functions -

  first frame (initializeFirstFrame, image_processor.cpp:337-352):
      good_features(max_features_num, 0.01, min_distance, user_mask)
  a publishing frame (findNewFeaturesToBeTracked, :1005-1037):
      mask = 255, a zeroed (2 min_distance + 1)^2 box around round(pt) of every live track, ANDed with the user mask;
      good_features(max_features_num - n_tracks, 0.01, min_distance, mask); a budget <= 0 gives the empty list
  any other frame runs no detection: the list is either consumed (trackNewFeatures appended it, :1001) or left as it was.

With an all-255 user mask the replay must reproduce lvo.Frontend.new_pts() byte for byte (tests/test_frontend_mask_replay.py proves
that on the CPU before the replay is used to judge the GPU).  Masks and sequences of the masked cases live here so that the CPU
suite (non-vacuity on the oracle alone) and the GPU suite use the same ones."""
import numpy as np

MM_ROWS = 4          # rows per workgroup of k_mask_max (larvio_amd/csrc/fe_image.hip): the strip seams the seam mask sits on


# ------------------------------------------------------------------ masks
def disc_mask(w, h, radius):
    """255 inside the centred disc (a fisheye's image circle), 0 in the vignette"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x - (w - 1) * 0.5) ** 2 + (y - (h - 1) * 0.5) ** 2 <= radius * radius, 255, 0).astype(np.uint8)


def half_plane_mask(w, h):
    """left half forbidden; the allowed side holds the values 1, 7 and 255 (any non-zero value allows)"""
    m = np.zeros((h, w), np.uint8)
    vals = np.array([1, 7, 255], np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    m[:, w // 2:] = vals[(x + 2 * y) % 3][:, w // 2:]
    return m


def block_mask(w, h, seed=5, block=16, keep=0.55):
    """random 16 x 16 blocks"""
    rng = np.random.default_rng(seed)
    g = (rng.random(((h + block - 1) // block, (w + block - 1) // block)) < keep).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:h, :w])


def seam_mask(w, h):
    """horizontal bands whose 0/255 edges sit on rows k MM_ROWS - 1, k MM_ROWS and k MM_ROWS + 1 in turn"""
    m = np.zeros((h, w), np.uint8)
    edges, k, off = [0], 6, 0
    while k * MM_ROWS + 1 < h:
        edges.append(k * MM_ROWS + (-1, 0, 1)[off % 3]); off += 1; k += 7
    edges.append(h)
    for j in range(len(edges) - 1):
        m[edges[j]:edges[j + 1]] = 255 if j % 2 else 0
    return m


def seam_rows(h):
    """the first row of every band of seam_mask (for the test that checks where the edges are)"""
    m = seam_mask(8, h)[:, 0]
    return [int(r) for r in np.nonzero(np.diff(m.astype(np.int32)))[0] + 1]


def zero_mask(w, h):
    return np.zeros((h, w), np.uint8)


# ------------------------------------------------------------------ sequences
def imu_for(seq, ts, n_hist=60):
    k0, k1 = seq.imu_index_range(-1.0, ts + 0.05)       # driver rule: samples with t < ts + 0.05 (larvioMain.cpp:98-102)
    return seq.imu_array(max(k1 - n_hist, 0), k1)


ODD_W, ODD_H, ODD_X0, ODD_Y0 = 301, 203, 200, 100


def sequence(name, count=None):
    """-> (frames [(ts, img)], imu sequence, front-end configuration) of a named stream:
    'headline'  752x480 radtan, CLAHE on, 150-feature budget (BASELINE.json's metric shape), 84 frames with the bootstrap
    'tumvi'     512x512 equidistant (BASELINE.json configs[3]'s shape), 300-feature budget, min_distance 15, from rest
    'odd'       301x203: a window cut out of the headline frames (principal point moved with it), neither size a multiple of 4"""
    from tests.conftest import synth_frames
    from larvio_amd import synthetic as S
    if name == "headline":
        frames = synth_frames(40, count or 84)
        return frames, S.imu_only_sequence(S.MASTER_SEED), S.frontend_config(max_features_num=150)
    if name == "tumvi":
        cam = dict(S.CAM_TUMVI_LIKE)
        frames = synth_frames(0, count or 64, cam=cam)
        return frames, S.imu_only_sequence(cam=cam), S.frontend_config(cam=cam, max_features_num=300, min_distance=15)
    if name == "odd":
        cam = dict(S.EUROC, width=ODD_W, height=ODD_H)
        fx, fy, cx, cy = S.EUROC["intrinsics"]
        cam["intrinsics"] = (fx, fy, cx - ODD_X0, cy - ODD_Y0)
        frames = [(t, np.ascontiguousarray(img[ODD_Y0:ODD_Y0 + ODD_H, ODD_X0:ODD_X0 + ODD_W])) for t, img in synth_frames(40, count or 64)]
        return frames, S.imu_only_sequence(S.MASTER_SEED), S.frontend_config(cam=cam, max_features_num=80, min_distance=10)
    raise ValueError(name)


def masked_cases():
    """(case id, sequence name, mask builder): every masked run of the GPU suite; the CPU suite asserts each is not vacuous"""
    return [
        ("headline-disc", "headline", lambda w, h: disc_mask(w, h, 230)),
        ("headline-halfplane", "headline", half_plane_mask),
        ("headline-blocks", "headline", block_mask),
        ("headline-seams", "headline", seam_mask),
        ("tumvi-disc250", "tumvi", lambda w, h: disc_mask(w, h, 250)),
        ("odd-seams", "odd", seam_mask),
        ("odd-blocks", "odd", block_mask),
    ]


# ------------------------------------------------------------------ the replay
def detector_image(cfg, img):
    """level 0 as the detector saw it: createImagePyramids (:318-334) equalises first when flag_equalize is set"""
    from oracle import lvo
    return lvo.clahe(img) if cfg["flag_equalize"] else np.ascontiguousarray(img, np.uint8)


def keep_out_mask(cfg, track_pts):
    """findNewFeaturesToBeTracked's own mask (:1009-1030): 255, a box of min_distance around round(pt) of every track zeroed;
    round() is C's, half away from zero"""
    w, h, md = cfg["width"], cfg["height"], cfg["min_distance"]
    m = np.full((h, w), 255, np.uint8)
    p = np.asarray(track_pts, np.float32).reshape(-1, 2).astype(np.float64)
    r = (np.sign(p) * np.floor(np.abs(p) + 0.5)).astype(np.int64)
    for rx, ry in r:
        r0, r1, c0, c1 = max(ry - md, 0), min(ry + md, h - 1), max(rx - md, 0), min(rx + md, w - 1)
        if r0 <= r1 and c0 <= c1:
            m[r0:r1 + 1, c0:c1 + 1] = 0
    return m


def replay_bootstrap(cfg, img, user_mask):
    from oracle import lvo
    pyr = lvo.LkPyramid(detector_image(cfg, img), cfg["patch_size"], cfg["pyramid_levels"])
    return pyr.good_features(cfg["max_features_num"], 0.01, float(cfg["min_distance"]), user_mask)


def replay_redetect(cfg, img, track_pts, user_mask):
    from oracle import lvo
    budget = cfg["max_features_num"] - len(track_pts)
    if budget <= 0:
        return np.zeros((0, 2), np.float32)
    m = keep_out_mask(cfg, track_pts)
    if user_mask is not None:
        m = np.where(np.asarray(user_mask) != 0, m, 0).astype(np.uint8)
    pyr = lvo.LkPyramid(detector_image(cfg, img), cfg["patch_size"], cfg["pyramid_levels"])
    return pyr.good_features(budget, 0.01, float(cfg["min_distance"]), m)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 2); b = np.ascontiguousarray(b, np.float32).reshape(-1, 2)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Replay:
    """Follows one front-end (the oracle's or the product's: both have .state, .tracks(), .new_pts()) frame by frame.

    before(fe) is called ahead of the frame, check(fe, img, have, user_mask) after it; check returns (kind, expected list) and
    raises AssertionError when the front-end's new points are not the replay's bits.  kind: 'bootstrap', 'redetect' or 'idle'."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.prev = np.zeros((0, 2), np.float32)
        self.frame = 0
        self.state_before = 1

    def before(self, fe):
        self.state_before = fe.state

    def check(self, fe, img, have, user_mask, imu_first_t=None, ts=None):
        got = fe.new_pts()
        where = "frame %d" % self.frame
        if self.state_before == 1:
            # (the very first call is skipped by the reference while the IMU buffer starts after the image, :134-142: the
            #  sequences here never do that, and the caller says so by passing the stamps)
            assert imu_first_t is None or imu_first_t <= ts, "the stream's first frame has no IMU sample before it"
            kind, want = "bootstrap", replay_bootstrap(self.cfg, img, user_mask)
            assert same_bits(got, want), (where, kind, len(got), len(want))
        elif have:
            kind, want = "redetect", replay_redetect(self.cfg, img, fe.tracks()["pts"], user_mask)
            assert same_bits(got, want), (where, kind, len(got), len(want))
        else:
            kind = "idle"
            want = got
            assert len(got) == 0 or same_bits(got, self.prev), (where, kind, len(got), len(self.prev))
        self.prev = np.array(want, np.float32, copy=True).reshape(-1, 2)
        self.frame += 1
        return kind, self.prev


def corners_in_forbidden_area(pts, mask):
    """how many of the corners sit (rounded) on a zero pixel of the mask"""
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    if not len(p):
        return 0
    x = np.rint(p[:, 0]).astype(np.int64); y = np.rint(p[:, 1]).astype(np.int64)      # corner coordinates are whole pixels
    return int((np.asarray(mask)[y, x] == 0).sum())
