"""CPU: the host helpers of larvio_amd.localize around ImageProcessor.build_map - MapCollector on a hand-made sequence of tracks()
dictionaries and export batches, and a save_map / load_map round trip."""
import numpy as np
import pytest

from larvio_amd.localize import MapCollector, save_map, load_map


def _tracks(ids, first_byte):
    d = np.zeros((len(ids), 32), np.uint8); d[:, 0] = first_byte; d[:, 1] = np.asarray(ids, np.uint8)
    return dict(ids=np.asarray(ids, np.uint64), desc=d, pts=np.zeros((len(ids), 2), np.float32))


def test_collector_joins_by_id():
    col = MapCollector()
    col.add_tracks(_tracks([1, 2, 3], 10))
    col.add_tracks(_tracks([2, 3, 4, 5], 20))                            # 2 and 3 keep the descriptor of the first frame
    col.add_tracks(_tracks([], 30))
    eye = np.eye(3)
    # the take_msckf_points form (with observation counts): 3, 9 (never tracked: no descriptor), 1
    col.add_points(np.array([3, 9, 1]), np.array([[3.0, 0, 0], [9.0, 0, 0], [1.0, 0, 0]]), np.stack([0.3 * eye, 0.9 * eye, 0.1 * eye]), np.array([7, 8, 9], np.int32))
    # the take_lost_features_cov form (none): 4, and 3 again with a smaller covariance, 1 again with a NaN one, 5 twice in one batch (equal traces: the first stays)
    nan = np.full((3, 3), np.nan)
    col.add_points(np.array([4, 3, 1, 5, 5]), np.array([[4.0, 0, 0], [3.5, 0, 0], [1.5, 0, 0], [5.0, 0, 0], [5.5, 0, 0]]), np.stack([0.4 * eye, 0.2 * eye, nan, 0.5 * eye, 0.5 * eye]))
    col.add_points(np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((0, 3, 3)))
    assert col.n_without_descriptor == 1
    ids, X, cov, desc, n_obs = col.arrays()
    assert ids.dtype == np.int64 and ids.tolist() == [3, 1, 4, 5]        # the order of the first export; 9 is left out, 2 was never exported
    assert X[:, 0].tolist() == [3.5, 1.0, 4.0, 5.0]                      # 3: the better copy; 1: the NaN copy lost; 5: the first of two equals
    assert np.allclose(cov[:, 0, 0], [0.2, 0.1, 0.4, 0.5]) and cov.shape == (4, 3, 3)
    assert n_obs.tolist() == [0, 9, 0, 0] and n_obs.dtype == np.int32
    assert desc.dtype == np.uint8 and desc[:, 0].tolist() == [10, 10, 20, 20] and desc[:, 1].tolist() == [3, 1, 4, 5]
    with pytest.raises(ValueError):
        col.add_points(np.array([1, 2]), np.zeros((1, 3)), np.zeros((1, 3, 3)))
    with pytest.raises(ValueError):
        col.add_tracks(dict(ids=np.array([1, 2], np.uint64), desc=np.zeros((1, 32), np.uint8)))


def test_an_empty_collector_gives_empty_arrays():
    ids, X, cov, desc, n_obs = MapCollector().arrays()
    assert ids.shape == (0,) and X.shape == (0, 3) and cov.shape == (0, 3, 3) and desc.shape == (0, 32) and n_obs.shape == (0,)


def test_save_load_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    n = 50
    ids = rng.permutation(1000)[:n].astype(np.int64); X = rng.normal(0, 1, (n, 3)); cov = rng.normal(0, 1, (n, 3, 3)); desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    order = rng.permutation(n)[:30].astype(np.int32)
    path = str(tmp_path / "map_without_suffix")
    save_map(path, ids, X, cov, desc, order)
    got = load_map(path)                                                 # the file is where it was asked for
    for a, b in zip(got, (ids, X, cov, desc, order)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    save_map(path, ids, X, None, desc)                                   # no covariances, the arrays are the map as they stand
    i2, X2, c2, d2, o2 = load_map(path)
    assert c2 is None and o2.tolist() == list(range(n)) and X2.tobytes() == X.tobytes()
    for bad in (np.array([0, 0]), np.array([n]), np.array([-1])):
        with pytest.raises(ValueError):
            save_map(path, ids, X, cov, desc, bad)
    with pytest.raises(ValueError):
        save_map(path, ids[:-1], X, cov, desc)
