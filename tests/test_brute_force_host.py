"""Host side of the brute-force searcher (no GPU): the config reader and its
dispatch, and the asset round trip of a brute-force searcher."""
import json
import os

import numpy as np
import pytest

from scann_amd import assets, config
from scann_amd.brute_force import BruteForceIndex
from scann_amd.index import METRIC_DOT, METRIC_SQUARED_L2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "builder_configs.json")


@pytest.fixture(scope="module")
def golden_text():
    with open(GOLDEN) as f:
        cases = {c["name"]: c for c in json.load(f)}
    return cases["brute_force"]["config"]


def test_golden_config_parses(golden_text):
    cfg = config.brute_force_config_from_text(golden_text)
    assert cfg == config.BruteForceConfig(num_neighbors=3, metric="squared_l2")
    assert config.is_brute_force(config.parse_text_proto(golden_text))


def test_tree_ah_reader_still_rejects(golden_text):
    with pytest.raises(ValueError, match="score_brute_force"):
        config.search_config_from_text(golden_text)


HEAD = 'num_neighbors: 3\ndistance_measure {distance_measure: "DotProductDistance"}\n'


@pytest.mark.parametrize("body", [
    "brute_force { fixed_point { enabled: true } }",
    "brute_force { bfloat16 { enabled: true } }",
    "partitioning { num_children: 10 }\nbrute_force { fixed_point { enabled: false } }",
])
def test_unsupported_brute_force_rejected(body):
    with pytest.raises(ValueError):
        config.brute_force_config_from_text(HEAD + body)


def test_plain_variants_accepted():
    for body in ("brute_force { fixed_point { enabled: false } }",
                 "brute_force { bfloat16 { enabled: False } }"):
        cfg = config.brute_force_config_from_text(HEAD + body)
        assert cfg == config.BruteForceConfig(num_neighbors=3, metric="dot_product")


def test_not_a_brute_force_config():
    with pytest.raises(ValueError):
        config.brute_force_config_from_text(HEAD)


@pytest.mark.parametrize("relative", [False, True])
def test_asset_round_trip(tmp_path, golden_text, relative):
    rng = np.random.default_rng(5)
    db = rng.standard_normal((37, 5)).astype(np.float32)
    db[3, 2] = -0.0
    index = BruteForceIndex(db, METRIC_SQUARED_L2)
    d = str(tmp_path / "bf")
    text = assets.save_brute_force_artifacts(index, golden_text, d, relative)
    assert sorted(os.listdir(d)) == ["dataset.npy", "scann_assets.pbtxt", "scann_config.pb"]
    assert "DATASET_NPY" in text
    assert assets.is_brute_force_artifacts(d)
    back, tree, cfg = assets.load_brute_force_artifacts(d)
    assert back.metric == METRIC_SQUARED_L2 and back.dim == 5 and back.num_datapoints == 37
    assert np.array_equal(back.dataset.view(np.uint32), db.view(np.uint32))
    assert cfg == config.brute_force_config_from_text(golden_text)
    # the decoded config prints as a config that parses to the same thing
    assert config.brute_force_config_from_text(assets.config_text(tree)) == cfg
    # the asset list passed explicitly, as ScannNumpy(artifacts_dir, assets_pbtxt) does
    again, _, _ = assets.load_brute_force_artifacts(d, text)
    assert np.array_equal(again.dataset, db)


def test_index_desc_and_checks():
    db = np.arange(12, dtype=np.float64).reshape(4, 3)
    index = BruteForceIndex(db, METRIC_DOT)
    assert index.dataset.dtype == np.float32 and index.dataset.flags.c_contiguous
    desc = index.desc()
    assert (desc.metric, desc.dim, desc.num_datapoints) == (METRIC_DOT, 3, 4)
    assert desc.dataset == index.dataset.ctypes.data
    with pytest.raises(ValueError):
        BruteForceIndex(np.zeros(3, np.float32), METRIC_DOT)
    with pytest.raises(ValueError):
        BruteForceIndex(np.zeros((2, 3), np.float32), 7)


def test_tree_ah_artifacts_are_not_brute_force(tmp_path):
    tree_cfg = HEAD + "partitioning { num_children: 10 }\n"
    d = tmp_path / "ah"
    d.mkdir()
    with open(d / "scann_config.pb", "wb") as f:
        f.write(assets.encode_message(config.parse_text_proto(tree_cfg), "ScannConfig"))
    assert not assets.is_brute_force_artifacts(str(d))
