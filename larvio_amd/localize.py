"""Localising against a prior map: the host steps around ImageProcessor.relocalise_map, ImageProcessor.align_landmarks,
ImageProcessor.match_landmarks and ImageProcessor.match_map (plain numpy, nothing here runs on the GPU).

Collect, build, save - in the session that maps:

    col = MapCollector()
    col.add_tracks(image_processor.tracks())                            # per frame: the first-seen descriptor of every feature id
    col.add_points(*larvio.take_msckf_points())                         # whenever: ids, positions, covariances (, observation counts)
    col.add_points(*larvio.take_lost_features_cov())
    ids, X, cov, desc, n_obs = col.arrays()                             # joined by id; an id without a descriptor is left out
    order, info = image_processor.build_map(X, cov, desc, max_score=0.05, r_dup=0.05)   # cull, dedupe and sort on the GPU; now resident
    save_map("map.npz", ids, X, cov, desc, order)                       # the raw arrays and the order: X[order] is the map

In the session that localises, keep the map on the device, best points first - once:

    ids, X, cov, desc, order = load_map("map.npz")
    X_map, cov_map, desc = X[order], cov[order], desc[order]
    image_processor.set_map(X_map, cov_map, desc)                       # up to 1,048,576 points
    sel = ops.map_select_options(max_r2=view_limit(fe_config))          # the guard against a radtan model folding back

A map from another session has its own origin and yaw (gravity fixes roll and pitch in both), so relocalise first - once, or whenever
the alignment is lost.  One call, whatever the map's size: the frame's corners are searched in the whole map, the best matches go to the
RANSAC over pairs:

    res, matches, info = image_processor.relocalise_map(R_wc, p_wc, ratio_pct=80)   # yaw and translation of the map
    p_w, cov_w = apply_alignment(res, X_map, cov_map)                   # the map in the filter's world frame (if res["status"] == ALIGN_OK)
    cov_psi_t = alignment_cov(res, sigma_px, fe_config)                 # sigma^2 A^-1 of (psi, t), if the caller wants it

For a map that is not resident (at most 1024 points a call), the same through the guided matcher:

    m0 = image_processor.match_landmarks(any_px, np.inf, desc, ratio_pct=80)   # an infinite radius: a global descriptor search
    am, idx = align_matches(m0, X_map)                                  # the OK records as (X, u, v)
    res, mask = image_processor.align_landmarks(am, R_wc, p_wc)

Then per frame to localise on, one call on the driver (VioDriver, VioDeferred; VioPipeline between drain() and the next step()):

    info = driver.localise_map(align=res, time=ts, sigma_px=sigma_px, select=sel)   # lvk_vio_localise_map: the filter's pose to a queued batch

It takes the camera pose of the frame's clone and its covariance from the filter on the device (lvk_ekf_camera_pose_cov: cov_cam in the
order [dtheta dp], rotation error on the camera side, dp in the world frame), projects the whole map, takes each search radius from the
point's and the pose's covariance, spreads its at most 1024 queries over a grid of image cells, matches them, gathers the matched points
and their covariances from the resident map into observation rows (lvk_map_gather_obs) and queues them on that clone; the host keeps no
copy of the map.  info holds the counts and the pose that was used.  The same link by hand, for a check:

    R_wc, p_wc, cov_cam = camera_pose_cov_ref(larvio.cov(), clone_col, clone, (R_b2c, t_c_b))   # or ops.camera_pose_cov on a device P
    rec, info = image_processor.match_map(R_wc, p_wc, align=res, cov_cam=cov_cam, select=sel)   # project, cull, pick <= 1024, match
    obs, idx = map_obs(rec, X_map, cov_map, res, sigma_px, fe_config)                          # the host-side check of lvk_map_gather_obs
    larvio.add_landmark_obs(obs["p_w"], obs["uv"], obs["sigma"], obs["cov_w"], time=ts)

And without a resident map, for a small map:

    px, ok = predict_pixels(p_w, R_wc, p_wc, fe_config)                # where the map's points should appear, from a pose prediction
    m = image_processor.match_landmarks(px[ok], radius, desc[ok])      # which corner of the frame each of them is
    obs, idx = landmark_obs(m, p_w[ok], cov_w[ok], sigma_px, fe_config)

A second session over the same site goes into the map of the first - its exports are in their own world frame, so it is aligned first
(found from the two maps' descriptors and points, or given: a session that was localised online holds the map's alignment into its
world, invert_alignment turns it round):

    used, order, info, minfo = image_processor.merge_map(X_b, cov_b, desc_b, r_dup=0.05)            # or align=invert_alignment(res)
    # used["status"] == ALIGN_OK: merged; order < old map_size: that resident point, else old map_size + B's index

align_points and merge_maps restate lvk_align_ransac_3d and the whole call in numpy - the judges of the tests, nothing to run per frame.

distort / project / predict_pixels are the forward camera model in numpy; the library's own is in lvk_map_select_queries."""
import numpy as np

from ._lib import MATCH_OK, ALIGN_MATCH
from .ops import LANDMARK_OBS


class MapCollector:
    """Joins, by feature id and over a whole session, what ImageProcessor.build_map needs: the descriptors come from tracks()["desc"] per
    frame (the first one seen per id stays), the positions and covariances from the batches of LarVio.take_lost_features_cov /
    take_msckf_points.  A point exported twice keeps the copy with the smaller covariance trace (a trace that is not finite loses, a tie
    keeps the earlier copy)."""

    def __init__(self):
        self._desc = {}                  # id -> (32,) uint8
        self._pts = {}                   # id -> (X, cov, n_obs), in the order of the first export

    def add_tracks(self, tracks):
        """tracks: what ImageProcessor.tracks() returned for a frame (its "ids" and "desc" are read)"""
        ids = np.asarray(tracks["ids"]).reshape(-1); desc = np.asarray(tracks["desc"], np.uint8).reshape(-1, 32)
        if len(ids) != len(desc):
            raise ValueError(f"{len(ids)} ids but {len(desc)} descriptors")
        for i, d in zip(ids, desc):
            self._desc.setdefault(int(i), d.copy())

    def add_points(self, ids, X, cov, n_obs=None):
        """one export batch: ids (n,), positions (n, 3), covariances (n, 3, 3), observation counts (n,) or None (recorded as 0)"""
        ids = np.asarray(ids).reshape(-1); X = np.asarray(X, np.float64).reshape(-1, 3); cov = np.asarray(cov, np.float64).reshape(-1, 3, 3)
        nob = np.zeros(len(ids), np.int32) if n_obs is None else np.asarray(n_obs, np.int32).reshape(-1)
        if not len(ids) == len(X) == len(cov) == len(nob):
            raise ValueError(f"{len(ids)} ids, {len(X)} positions, {len(cov)} covariances, {len(nob)} observation counts")

        def trace(c):
            t = float(c[0, 0] + c[1, 1] + c[2, 2])
            return t if np.isfinite(t) else np.inf
        for i, x, c, k in zip(ids, X, cov, nob):
            old = self._pts.get(int(i))
            if old is None or trace(c) < trace(old[1]):
                self._pts[int(i)] = (x.copy(), c.copy(), int(k))

    @property
    def n_without_descriptor(self):
        """exported points whose id no add_tracks call has seen: arrays() leaves them out"""
        return sum(1 for i in self._pts if i not in self._desc)

    def arrays(self):
        """-> (ids (n,) int64, X (n, 3), cov (n, 3, 3), desc (n, 32) uint8, n_obs (n,) int32) of the ids that have both a position and a
        descriptor, in the order of their first export"""
        keep = [i for i in self._pts if i in self._desc]
        n = len(keep)
        ids = np.array(keep, np.int64).reshape(n)
        X = np.array([self._pts[i][0] for i in keep], np.float64).reshape(n, 3)
        cov = np.array([self._pts[i][1] for i in keep], np.float64).reshape(n, 3, 3)
        desc = np.array([self._desc[i] for i in keep], np.uint8).reshape(n, 32)
        n_obs = np.array([self._pts[i][2] for i in keep], np.int32).reshape(n)
        return ids, X, cov, desc, n_obs


def save_map(path, ids, X, cov, desc, order=None):
    """One .npz with ids, X, cov, desc and order: the raw arrays as MapCollector.arrays() gave them and the order ImageProcessor.build_map
    returned (None: the arrays are the map as they stand, order = 0 .. n - 1); cov None is stored as an empty array.  The file is written
    at `path` exactly (numpy adds no suffix)."""
    X = np.asarray(X, np.float64).reshape(-1, 3); n = len(X)
    ids = np.asarray(ids, np.int64).reshape(-1); desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    cov = np.zeros((0, 3, 3)) if cov is None else np.asarray(cov, np.float64).reshape(-1, 3, 3)
    order = np.arange(n, dtype=np.int32) if order is None else np.asarray(order, np.int32).reshape(-1)
    if len(ids) != n or len(desc) != n or len(cov) not in (0, n):
        raise ValueError(f"{n} points but {len(ids)} ids, {len(desc)} descriptors, {len(cov)} covariances")
    if len(order) and (order.min() < 0 or order.max() >= n or len(np.unique(order)) != len(order)):
        raise ValueError("order must hold distinct indices into the arrays")
    with open(path, "wb") as f:
        np.savez(f, ids=ids, X=X, cov=cov, desc=desc, order=order)


def load_map(path):
    """-> (ids, X, cov or None, desc, order) as save_map stored them: X[order], cov[order], desc[order] is what set_map takes"""
    with np.load(path, allow_pickle=False) as z:
        ids, X, cov, desc, order = (z[k] for k in ("ids", "X", "cov", "desc", "order"))
    return ids, X, (cov if len(cov) == len(X) and len(X) else None), desc, order


def distort(xy, model, dist):
    """forward distortion of normalised image coordinates (n, 2): model 0 = radtan (k1, k2, p1, p2), 1 = equidistant (k1..k4)"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    r2 = x * x + y * y
    if model == 0:
        k1, k2, p1, p2 = dist
        rad = 1.0 + (k2 * r2 + k1) * r2
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    elif model == 1:
        r = np.sqrt(r2)
        th = np.arctan(r); t2 = th * th
        thd = th * (1.0 + t2 * (dist[0] + t2 * (dist[1] + t2 * (dist[2] + t2 * dist[3]))))
        s = np.where(r > 1e-8, thd / np.maximum(r, 1e-300), 1.0)
        xd, yd = x * s, y * s
    else:
        raise ValueError("distortion_model must be 0 (radtan) or 1 (equidistant)")
    return np.stack([xd, yd], -1)


def project(xy, fe_config):
    """normalised undistorted coordinates (n, 2) -> pixels (n, 2) float64 of the configured camera"""
    fx, fy, cx, cy = fe_config["intrinsics"]
    d = distort(xy, fe_config["distortion_model"], fe_config["distortion"])
    return np.stack([fx * d[:, 0] + cx, fy * d[:, 1] + cy], -1)


def predict_pixels(p_w, R_wc, p_wc, fe_config, min_depth=0.1):
    """World points p_w (n, 3) seen from the camera pose (R_wc: camera-to-world rotation, p_wc: camera position in the world) through the
    front-end's camera (fe_config: the ImageProcessor's configuration dict).  -> (pixels (n, 2) float32, ok (n,) bool); ok is False for a
    point behind the camera (depth <= min_depth) or outside the image - its pixel is NaN, which match_landmarks answers with NO_CANDIDATE."""
    p_w = np.asarray(p_w, np.float64).reshape(-1, 3)
    p_c = (p_w - np.asarray(p_wc, np.float64).reshape(1, 3)) @ np.asarray(R_wc, np.float64).reshape(3, 3)      # rows: R_wc^T (p_w - p_wc)
    front = p_c[:, 2] > min_depth
    z = np.where(front, p_c[:, 2], 1.0)
    px = project(p_c[:, :2] / z[:, None], fe_config)
    ok = front & (px[:, 0] >= 0) & (px[:, 0] <= fe_config["width"] - 1) & (px[:, 1] >= 0) & (px[:, 1] <= fe_config["height"] - 1)
    px[~ok] = np.nan
    return px.astype(np.float32), ok


def landmark_obs(matches, p_w, cov_w, sigma_px, fe_config):
    """The observation rows of the matches whose status is MATCH_OK.  matches: what match_landmarks returned for the points p_w (n, 3) with
    covariances cov_w (None, one 3 x 3, or n of them); sigma_px: the standard deviation of a matched corner in pixels, turned into
    normalised units with the mean focal length of fe_config.  -> (obs: an ops.LANDMARK_OBS array (p_w, cov_w, uv, sigma), idx: the rows of
    `matches` they came from); feed obs["p_w"], obs["uv"], obs["sigma"], obs["cov_w"] to LarVio.add_landmark_obs."""
    p_w = np.asarray(p_w, np.float64).reshape(-1, 3)
    if len(matches) != len(p_w):
        raise ValueError(f"{len(matches)} matches for {len(p_w)} points")
    idx = np.nonzero(matches["status"] == MATCH_OK)[0]
    fx, fy = fe_config["intrinsics"][:2]
    obs = np.zeros(len(idx), LANDMARK_OBS)
    obs["p_w"] = p_w[idx]
    obs["uv"] = matches["und"][idx].astype(np.float64)
    obs["sigma"] = float(sigma_px) / (0.5 * (fx + fy))
    if cov_w is not None:
        c = np.asarray(cov_w, np.float64)
        obs["cov_w"] = c.reshape(1, 9) if c.size == 9 else c.reshape(-1, 9)[idx]
    return obs, idx


def map_obs(records, X_map, cov_map, result, sigma_px, fe_config):
    """The observation rows of match_map's records whose match is MATCH_OK.  records: the MAP_MATCH array match_map returned for the map
    X_map (n, 3) with covariances cov_map (None, one 3 x 3, or n of them), both in the map's own frame; result: the alignment match_map
    was given (an ALIGN_RESULT record, or None for a map already in the world frame) - it is applied to X[index] and cov[index];
    sigma_px as landmark_obs takes it.  -> (obs: an ops.LANDMARK_OBS array, idx: the rows of `records` they came from)"""
    X_map = np.asarray(X_map, np.float64).reshape(-1, 3)
    idx = np.nonzero(records["m"]["status"] == MATCH_OK)[0]
    k = records["index"][idx]
    cov = None if cov_map is None else np.asarray(cov_map, np.float64)
    if cov is not None:
        cov = cov.reshape(1, 3, 3) if cov.size == 9 else cov.reshape(-1, 3, 3)[k]
    if result is None:
        p_w, cov_w = X_map[k], cov
    else:
        p_w, cov_w = apply_alignment(result, X_map[k], cov)
    fx, fy = fe_config["intrinsics"][:2]
    obs = np.zeros(len(idx), LANDMARK_OBS)
    obs["p_w"] = p_w
    obs["uv"] = records["m"]["und"][idx].astype(np.float64)
    obs["sigma"] = float(sigma_px) / (0.5 * (fx + fy))
    if cov_w is not None:
        obs["cov_w"] = cov_w.reshape(-1, 9)
    return obs, idx


def _quat_to_rot(q):
    """R(q), q = [x y z w], in the order lvk_ekf_camera_pose_cov states (Eigen's Quaternion::toRotationMatrix)"""
    x, y, z, w = (np.float64(v) for v in np.asarray(q, np.float64).reshape(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]], np.float64)


def camera_pose(clone, extrinsics):
    """The camera pose of a clone of the filter's window, bit for bit as lvk_ekf_camera_pose_cov forms it.  clone: a record with q ([x y z w],
    body to world) and p (one entry of LarVio.clones()); extrinsics: (R_b2c (3, 3), t_c_b (3,)) as the filter's state hands them out.
    -> (R_wc = R_b R_b2c^T (3, 3), p_wc = p_b + R_b t_c_b (3,))"""
    Rb = _quat_to_rot(clone["q"]); pb = np.asarray(clone["p"], np.float64).reshape(3)
    Re = np.asarray(extrinsics[0], np.float64).reshape(3, 3); t = np.asarray(extrinsics[1], np.float64).reshape(3)
    R_wc = np.empty((3, 3)); p_wc = np.empty(3)
    for i in range(3):
        for j in range(3):
            R_wc[i, j] = (Rb[i, 0] * Re[j, 0] + Rb[i, 1] * Re[j, 1]) + Rb[i, 2] * Re[j, 2]
        p_wc[i] = pb[i] + ((Rb[i, 0] * t[0] + Rb[i, 1] * t[1]) + Rb[i, 2] * t[2])
    return R_wc, p_wc


def camera_pose_cov_ref(P, clone_col, clone, extrinsics):
    """The numpy restatement of lvk_ekf_camera_pose_cov (include/lvk_c.h), expression by expression in the order stated there - for a
    check, or where the covariance is on the host anyway (LarVio.cov()).  P: the filter's covariance (n, n); clone_col: the first of the
    clone's six columns (leg_dim + 6 * its rank in the window); clone, extrinsics as camera_pose takes them.
    -> (R_wc (3, 3), p_wc (3,), cov_cam (6, 6) in the order [dtheta dp], rotation error on the camera side, dp in the world frame)"""
    P = np.asarray(P, np.float64)
    R_wc, p_wc = camera_pose(clone, extrinsics)
    Rb = _quat_to_rot(clone["q"]); Re = np.asarray(extrinsics[0], np.float64).reshape(3, 3)
    u = p_wc * 0.0
    t = np.asarray(extrinsics[1], np.float64).reshape(3)
    for i in range(3):
        u[i] = (Rb[i, 0] * t[0] + Rb[i, 1] * t[1]) + Rb[i, 2] * t[2]
    J = np.zeros((6, 12))
    J[0:3, 0:3] = Re; J[0:3, 6:9] = R_wc.T; J[3:6, 3:6] = Rb
    J[3:6, 6:9] = np.array([[0.0, u[2], -u[1]], [-u[2], 0.0, u[0]], [u[1], -u[0], 0.0]])
    J[3:6, 9:12] = np.eye(3)
    cols = np.r_[15:21, int(clone_col):int(clone_col) + 6]
    Ps = P[np.ix_(cols, cols)]
    T = np.zeros((6, 12))
    for l in range(12):
        T = T + J[:, l:l + 1] * Ps[l:l + 1, :]
    cov = np.zeros((6, 6))
    for l in range(12):
        cov = cov + T[:, l:l + 1] * J[:, l:l + 1].T
    cov = np.triu(cov) + np.triu(cov, 1).T
    return R_wc, p_wc, cov


def view_limit(fe_config, r_max=20.0, step=0.01):
    """The value to pass as max_r2 to match_map / ops.map_select_queries: the largest r2 = x^2 + y^2 of a normalised point, along the rays
    from the principal point towards the four image corners and the four edge midpoints, up to which the forward model is still
    increasing (the distorted radius grows with the undistorted one) and lands inside the image.  Beyond it a radtan model with a
    negative k1 folds back and can put a point far outside the field of view into the image.  Found per ray by a scan in steps of
    `step` up to the radius r_max and then bisection on `distort`; the largest of the eight."""
    fx, fy, cx, cy = fe_config["intrinsics"]
    w, h = fe_config["width"], fe_config["height"]
    model, dist = fe_config["distortion_model"], fe_config["distortion"]
    best = 0.0
    for u, v in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0.5 * (w - 1), 0), (0.5 * (w - 1), h - 1), (0, 0.5 * (h - 1)), (w - 1, 0.5 * (h - 1))):
        d = np.array([(u - cx) / fx, (v - cy) / fy])
        nd = float(np.linalg.norm(d))
        if nd == 0.0:
            continue
        d = d / nd

        def good(rho):
            a = distort(rho * d, model, dist)[0]; b = distort(rho * (1.0 + 1e-6) * d, model, dist)[0]
            px, py = fx * a[0] + cx, fy * a[1] + cy
            return bool(np.hypot(*b) > np.hypot(*a) and 0 <= px <= w - 1 and 0 <= py <= h - 1)
        lo, hi = 0.0, None
        for k in range(1, int(round(r_max / step)) + 1):
            if not good(k * step):
                hi = k * step
                break
            lo = k * step
        if hi is not None:
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if good(mid) else (lo, mid)
        best = max(best, lo * lo)
    return best


def align_matches(matches, X_map):
    """The ALIGN_MATCH records (X, u, v) of the matches whose status is MATCH_OK.  matches: what match_landmarks (or ops.orb_match_guided
    with `und` filled in) returned for the map points X_map (n, 3), in the map's own frame.  -> (records, idx: the rows they came from)"""
    X_map = np.asarray(X_map, np.float64).reshape(-1, 3)
    if len(matches) != len(X_map):
        raise ValueError(f"{len(matches)} matches for {len(X_map)} points")
    idx = np.nonzero(matches["status"] == MATCH_OK)[0]
    out = np.zeros(len(idx), ALIGN_MATCH)
    out["X"] = X_map[idx]
    out["u"] = matches["und"][idx, 0].astype(np.float64); out["v"] = matches["und"][idx, 1].astype(np.float64)
    return out, idx


def apply_alignment(result, X_map, cov_map=None):
    """p_w = Rz X + t for the map points X_map (n, 3) with the refined (c, s, t) of an ALIGN_RESULT record, and their covariances
    (None, one 3 x 3 or n of them) rotated by Rz: what predict_pixels and landmark_obs take.  -> (p_w (n, 3), cov_w (n, 3, 3) or None).
    p_w is formed by the expressions lvk_map_select_queries and lvk_map_gather_obs state - q = (c X_x - s X_y, s X_x + c X_y),
    p_w = (q_x + t_x, q_y + t_y, X_z + t_z) -, so it is bit for bit the point the library projects and fuses; the covariance goes through
    numpy's matrix product and has no fixed order."""
    c, s = np.float64(result["c"]), np.float64(result["s"])
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    X_map = np.asarray(X_map, np.float64).reshape(-1, 3)
    t = np.asarray(result["t"], np.float64).reshape(3)
    p_w = np.stack([(c * X_map[:, 0] - s * X_map[:, 1]) + t[0], (s * X_map[:, 0] + c * X_map[:, 1]) + t[1], X_map[:, 2] + t[2]], -1)
    if cov_map is None:
        return p_w, None
    cov = np.asarray(cov_map, np.float64).reshape(-1, 3, 3)
    return p_w, Rz @ cov @ Rz.T


def alignment_cov(result, sigma_px, fe_config):
    """sigma^2 A^-1: the covariance of (psi, t_x, t_y, t_z) from the refinement's normal matrix, for corners with a standard deviation of
    sigma_px pixels (turned into normalised units with the mean focal length of fe_config, as landmark_obs does)"""
    fx, fy = fe_config["intrinsics"][:2]
    sigma = float(sigma_px) / (0.5 * (fx + fy))
    return sigma * sigma * np.linalg.inv(np.asarray(result["A"], np.float64).reshape(4, 4))


def invert_alignment(result):
    """lvk_align_invert in numpy: (c, s, t) of Y = Rz X + t the other way round, by the header's expressions -> (c', s', t')"""
    c, s = np.float64(result["c"]), np.float64(result["s"])
    t = np.asarray(result["t"], np.float64).reshape(3)
    return c, -s, np.array([-(c * t[0] + s * t[1]), -(c * t[1] - s * t[0]), -t[2]])


def transform_points(X, cov=None, align=None, cov_align=None):
    """lvk_map_transform in numpy, every expression in the header's order, so the result is the library's bit for bit.  X (n, 3), cov
    (n, 3, 3) or None, align: None or a record / dict with c, s, t, cov_align: None or 4 x 4.  -> (p (n, 3), cov' (n, 3, 3) or None)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    c, s, t = (np.float64(1.0), np.float64(0.0), np.zeros(3)) if align is None else (np.float64(align["c"]), np.float64(align["s"]), np.asarray(align["t"], np.float64).reshape(3))
    with np.errstate(all="ignore"):
        q0 = c * X[:, 0] - s * X[:, 1]; q1 = s * X[:, 0] + c * X[:, 1]
        p = np.stack([q0 + t[0], q1 + t[1], X[:, 2] + t[2]], -1)
        if cov is None and cov_align is None:
            return p, None
        w = {}
        if cov is not None:
            S = np.asarray(cov, np.float64).reshape(-1, 3, 3)
            a, b, d, e, f, g = S[:, 0, 0], S[:, 0, 1], S[:, 1, 1], S[:, 0, 2], S[:, 1, 2], S[:, 2, 2]
            m00 = c * a - s * b; m01 = c * b - s * d; m10 = s * a + c * b; m11 = s * b + c * d
            w = {(0, 0): m00 * c - m01 * s, (0, 1): m00 * s + m01 * c, (1, 1): m10 * s + m11 * c, (0, 2): c * e - s * f, (1, 2): s * e + c * f, (2, 2): g.copy()}
        if cov_align is not None:
            P = np.asarray(cov_align, np.float64).reshape(4, 4)
            j = [-q1, q0, np.zeros(len(X))]
            for r in range(3):
                for u in range(r, 3):
                    k = (((j[r] * j[u]) * P[0, 0] + j[r] * P[0, 1 + u]) + j[u] * P[0, 1 + r]) + P[1 + r, 1 + u]
                    w[r, u] = w[r, u] + k if cov is not None else k
        out = np.zeros((len(X), 3, 3))
        for (r, u), v in w.items():
            out[:, r, u] = v; out[:, u, r] = v
    return p, out


ALIGN3D_DEFAULTS = dict(thresh=0.10, min_rho=0.5, min_inliers=6)


def align_points(X, Y, pairs, thresh=0.0, min_rho=0.0, min_inliers=0):
    """lvk_align_ransac_3d in numpy float64, every expression in the header's order: the hypotheses, their counts, the winner and its mask
    are the library's bit for bit; the refinement's sums run in numpy's order, so c, s, t, A and rms agree to rounding.  X, Y (n, 3):
    the matched points in B's and in the map's frame; pairs (P, 2).  -> dict(status, hyp, n_inliers, mask, c, s, t, c0, s0, t0, A, rms,
    n_models (P,), count (P,), hc, hs (P,), ht (P, 3))"""
    thresh = np.float64(thresh or ALIGN3D_DEFAULTS["thresh"]); min_rho = np.float64(min_rho or ALIGN3D_DEFAULTS["min_rho"]); min_inliers = int(min_inliers or ALIGN3D_DEFAULTS["min_inliers"])
    X = np.asarray(X, np.float64).reshape(-1, 3); Y = np.asarray(Y, np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n, P = len(X), len(pairs)
    out = dict(status=1, hyp=-1, n_inliers=0, mask=np.zeros(n, np.uint8), c=np.float64(1), s=np.float64(0), t=np.zeros(3), c0=np.float64(1), s0=np.float64(0), t0=np.zeros(3),
               A=np.zeros((4, 4)), rms=np.float64(0), n_models=np.zeros(P, np.int32), count=np.zeros(P, np.int32), hc=np.zeros(P), hs=np.zeros(P), ht=np.zeros((P, 3)))
    if n < 2 or P == 0:
        return out
    thresh2 = thresh * thresh; two = 2.0 * thresh; rho2 = min_rho * min_rho
    i, j = pairs[:, 0], pairs[:, 1]
    ok = (i != j) & (i >= 0) & (j >= 0) & (i < n) & (j < n)
    ii, jj = np.where(ok, i, 0), np.where(ok, j, 0)
    with np.errstate(all="ignore"):
        a = X[ii] - X[jj]; b = Y[ii] - Y[jj]
        ra2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]; rb2 = b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]
        ok &= (ra2 > rho2) & (rb2 > rho2)
        ok &= ~(np.abs(a[:, 2] - b[:, 2]) > two)
        ok &= ~(np.abs(np.sqrt(ra2) - np.sqrt(rb2)) > two)
        dot = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]; crs = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        nrm = np.sqrt(dot * dot + crs * crs)
        ok &= nrm > 0
        c = dot / nrm; s = crs / nrm
        qi0 = c * X[ii, 0] - s * X[ii, 1]; qi1 = s * X[ii, 0] + c * X[ii, 1]
        qj0 = c * X[jj, 0] - s * X[jj, 1]; qj1 = s * X[jj, 0] + c * X[jj, 1]
        t = np.stack([((Y[ii, 0] - qi0) + (Y[jj, 0] - qj0)) / 2.0, ((Y[ii, 1] - qi1) + (Y[jj, 1] - qj1)) / 2.0, ((Y[ii, 2] - X[ii, 2]) + (Y[jj, 2] - X[jj, 2])) / 2.0], -1)

        def inliers(c, s, t):
            q0 = c[:, None] * X[None, :, 0] - s[:, None] * X[None, :, 1]; q1 = s[:, None] * X[None, :, 0] + c[:, None] * X[None, :, 1]
            dx = (q0 + t[:, 0, None]) - Y[None, :, 0]; dy = (q1 + t[:, 1, None]) - Y[None, :, 1]; dz = (X[None, :, 2] + t[:, 2, None]) - Y[None, :, 2]
            return ((dx * dx + dy * dy) + dz * dz) <= thresh2
        hs_ = np.nonzero(ok)[0]
        count = np.zeros(P, np.int64)
        for lo in range(0, len(hs_), 256):
            sl = hs_[lo:lo + 256]
            count[sl] = inliers(c[sl], s[sl], t[sl]).sum(1)
    out["n_models"] = ok.astype(np.int32); out["count"] = count.astype(np.int32)
    out["hc"] = np.where(ok, c, 0.0); out["hs"] = np.where(ok, s, 0.0); out["ht"] = np.where(ok[:, None], t, 0.0)
    if not ok.any():
        return out
    w = int(hs_[np.argmax(count[hs_])])                  # the first of the largest: ties to the lowest hypothesis
    with np.errstate(all="ignore"):
        mask = inliers(c[w:w + 1], s[w:w + 1], t[w:w + 1])[0]
    m = int(count[w])
    out.update(hyp=w, n_inliers=m, mask=mask.astype(np.uint8), c=c[w], s=s[w], t=t[w].copy(), c0=c[w], s0=s[w], t0=t[w].copy(), status=2)
    if m < min_inliers:
        return out
    Xi, Yi = X[mask], Y[mask]
    cnt = np.float64(m)
    mX = Xi.sum(0) / cnt; mY = Yi.sum(0) / cnt
    x = Xi[:, :2] - mX[:2]; y = Yi[:, :2] - mY[:2]
    D = (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]).sum(); C = (x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]).sum()
    W = ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1])).sum()
    nr = np.sqrt(D * D + C * C)
    cr, sr, tr, status = c[w], s[w], t[w].copy(), 3
    if nr > 1e-12 * (W / 2.0):
        status = 0
        cr = D / nr; sr = C / nr
        tr = np.array([mY[0] - (cr * mX[0] - sr * mX[1]), mY[1] - (sr * mX[0] + cr * mX[1]), mY[2] - mX[2]])
    q0 = cr * Xi[:, 0] - sr * Xi[:, 1]; q1 = sr * Xi[:, 0] + cr * Xi[:, 1]
    rx = (q0 + tr[0]) - Yi[:, 0]; ry = (q1 + tr[1]) - Yi[:, 1]; rz = (Xi[:, 2] + tr[2]) - Yi[:, 2]
    A = np.zeros((4, 4))
    A[0, 0] = (q1 * q1 + q0 * q0).sum(); A[0, 1] = A[1, 0] = (-q1).sum(); A[0, 2] = A[2, 0] = q0.sum(); A[1, 1] = A[2, 2] = A[3, 3] = cnt
    out.update(status=status, c=cr, s=sr, t=tr, A=A, rms=np.sqrt(((rx * rx + ry * ry) + rz * rz).sum() / cnt))
    return out


def merge_maps(A, B, align=None, cov_align=None, max_dist=58, ratio_pct=100, thresh=0.0, min_rho=0.0, min_inliers=0, max_hypotheses=0, seed=0, build=None, match=None,
               **build_options):
    """lvk_frontend_merge_map in numpy: the judge of ImageProcessor.merge_map.  A, B: (X, cov, desc) of the resident map and of the new
    session; align: None (find it) or a record / dict with c, s, t (B -> A).  build, match: the restatements of lvk_map_build and
    lvk_orb_match_global - by default tests/map_build_ref.build and tests/orb_global_ref.match of the source tree.
    -> dict(align: align_points' dict (or status 0 and the given c, s, t), merged: bool, order: the merged map in the caller's view, X,
    cov, desc: the merged map, info, match_info (None when align was given), order_B, matches: (B sorted index, A index) pairs, matches_X, matches_Y, pairs: what the 3D alignment was given)"""
    from .ops import align_draw_pairs
    if build is None or match is None:
        try:
            from tests.map_build_ref import build as ref_build
            from tests.orb_global_ref import match as ref_match
        except ImportError as e:
            raise ImportError("larvio_amd.localize.merge_maps takes its restatements of lvk_map_build and lvk_orb_match_global from tests/map_build_ref.py and "
                              "tests/orb_global_ref.py of the source tree, which is not on sys.path here: run from the repository's root, or pass build= and match=") from e
        build = build or ref_build; match = match or ref_match
    XA, covA, descA = (np.asarray(A[0], np.float64).reshape(-1, 3), np.asarray(A[1], np.float64).reshape(-1, 3, 3), np.asarray(A[2], np.uint8).reshape(-1, 32))
    nA = len(XA)
    rb = build(B[0], B[1], B[2], None, **build_options)
    out = dict(merged=False, order_B=rb["order"], match_info=None, matches=np.zeros((0, 2), np.int64), order=None, X=None, cov=None, desc=None, info=None)
    if align is None:
        nq = min(len(rb["order"]), 4096)
        g = match(descA, rb["desc"][:nq], max_dist, ratio_pct, 1024)
        sel = g["sel"]
        pr = align_draw_pairs(len(sel), max_hypotheses, seed)
        al = align_points(rb["X"][sel["cand"]], XA[sel["index"]], np.stack([pr["i"], pr["j"]], 1).reshape(-1, 2), thresh, min_rho, min_inliers)
        out.update(align=al, match_info=g["info"], matches=np.stack([sel["cand"], sel["index"]], 1).astype(np.int64).reshape(-1, 2), matches_X=rb["X"][sel["cand"]],
                   matches_Y=XA[sel["index"]], pairs=np.stack([pr["i"], pr["j"]], 1).reshape(-1, 2))
        if al["status"] != 0:
            return out
    else:
        al = dict(status=0, c=np.float64(align["c"]), s=np.float64(align["s"]), t=np.asarray(align["t"], np.float64).reshape(3).copy())
        out["align"] = al
    pB, covB = transform_points(rb["X"], rb["cov"], al, cov_align)
    rm = build(np.concatenate([XA, pB]), np.concatenate([covA, covB]), np.concatenate([descA, rb["desc"]]), None, **build_options)
    o = rm["order"].astype(np.int64)
    order = np.where(o < nA, o, nA + rb["order"].astype(np.int64)[np.maximum(o - nA, 0)]).astype(np.int32) if len(rb["order"]) else o.astype(np.int32)
    out.update(merged=True, order=order, X=rm["X"], cov=rm["cov"], desc=rm["desc"], info=rm["info"])
    return out
