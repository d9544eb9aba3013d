"""lib.datasets on the CPU: the random stream and the records of ``ObjectPoseDataset.__getitem__`` against the
reference's own ``__getitem__`` (tests/golden/dataset_ref.npz, and live where the reference tree is present), the
tracking task's previous frame, discovery, and the collate function."""
import json
import os

import numpy as np
import pytest
import torch

from centerpose_amd.pose_targets import pack_annotations
from centerpose_amd.pose_targets_track import pack_track_annotations
from centerpose_amd.train_inputs import pack_input
from tests import dataset_cases as DC
from tests import pose_target_cases as PC

needs_reference = pytest.mark.skipif(not PC.reference_available(), reason="the reference tree is not present")


@pytest.fixture(scope="module")
def golden():
    return np.load(DC.GOLDEN)


def _same_capture(a, b):
    for k in a:
        if k in ("color", "color_pre"):
            assert (a[k] is None) == (b[k] is None), k
            if a[k] is not None:
                assert a[k]["order"] == b[k]["order"] and list(a[k]["alphas"]) == list(b[k]["alphas"])
                assert np.array_equal(a[k]["light"], b[k]["light"])
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _check_single(name, cap):
    """The new dataset's sample equals the packers applied to the reference's captured values, exactly in float64, and
    leaves the three generators where the reference leaves them."""
    opt, anns, w, h, _, split = DC.case(name)
    sample, states = DC.dataset_run(name)
    assert (cap["width"], cap["height"]) == (w, h)
    want = pack_annotations(anns, cap["trans_output_rot"], w, h, cap["flipped"], cap["rot"], opt)
    want.update(pack_input(cap["trans_input"], h, w, cap["flipped"], cap["color"]))
    assert sorted(sample) == ["frame", "pt_image", "pt_objects", "ti_image"]
    for k, v in want.items():
        assert sample[k].dtype == np.float64 and np.array_equal(sample[k], v), (name, k)
    assert sample["frame"].dtype == np.uint8 and sample["frame"].shape == (h, w, 3) and not sample["frame"].any()
    assert states == cap["states"], name
    if split == "val":
        assert cap["color"] is None and not cap["flipped"] and cap["rot"] == 0


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_random_stream_and_records_golden(name, golden):
    _check_single(name, DC.from_golden(golden, name))


@needs_reference
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_random_stream_and_records_live(name, golden):
    cap = DC.reference_run(name)
    _same_capture(DC.from_golden(golden, name), cap)  # the golden file is the reference's answer
    _check_single(name, cap)


def test_cases_cover_the_branches(golden):
    """The cases reach both sides of every draw-dependent branch: flipped and not, rotated and not, colour and not."""
    caps = [DC.from_golden(golden, n) for n in DC.CASES]
    train = [c for n, c in zip(DC.CASES, caps) if DC.CASES[n][2] == "train"]
    assert {c["flipped"] for c in train} == {True, False}
    assert {c["rot"] != 0 for c in train} == {True, False}
    assert {c["color"] is None for c in train} == {True, False}
    half = [c for n, c in zip(DC.CASES, caps) if DC.CASES[n][3]["flip"] == 0.5 and DC.CASES[n][2] == "train"]
    assert {c["flipped"] for c in half} == {True, False}  # the draw decides, not the option


def _check_track(name, cap):
    opt, anns, pre, w, h, _, _ = DC.track_case(name)
    sample, states, draws = DC.dataset_track_run(name)
    assert states == cap["states"], name  # the stream up to the point where the noise draws begin
    same = bool(opt.same_aug_pre)  # the previous frame is one frame away
    assert np.array_equal(cap["trans_input"], cap["trans_input_pre"]) == same
    want = pack_track_annotations(anns, pre, cap["trans_output_rot"], cap["trans_input_pre"], w, h, cap["flipped"], cap["rot"],
                                  opt, draws)
    want.update(pack_input(cap["trans_input"], h, w, cap["flipped"], cap["color"]))
    want["ti_image_pre"] = pack_input(cap["trans_input_pre"], h, w, cap["flipped"], cap["color_pre"])["ti_image"]
    assert sorted(sample) == sorted(list(want) + ["frame", "frame_pre"])
    for k, v in want.items():
        assert np.array_equal(sample[k], v), (name, k)
    assert draws.shape == (len(pre["objects"]), 65)


@pytest.mark.parametrize("name", sorted(DC.TRACK_CASES))
def test_tracking_task_golden(name, golden):
    _check_track(name, DC.from_golden(golden, name))


@needs_reference
@pytest.mark.parametrize("name", sorted(DC.TRACK_CASES))
def test_tracking_task_live(name, golden):
    cap = DC.reference_track_run(name)
    _same_capture(DC.from_golden(golden, name), cap)
    _check_track(name, cap)


def test_generation_records():
    """With opt.data_generation_mode_ratio > 0 every sample carries ptk_gen / ptk_det_meta, built from the drawn mode and
    the previous frame's own augmentation."""
    import tempfile

    from centerpose_amd.lib.datasets import dataset_combined as M

    opt, anns, pre, w, h, seed, _ = DC.track_case("track_own_aug")
    opt.data_generation_mode_ratio = 1.0
    for a in (anns, pre):
        a["camera_data"]["intrinsics"] = {"fx": 500.0, "fy": 510.0, "cx": w / 2.0, "cy": h / 2.0}
    with tempfile.TemporaryDirectory() as tmp:
        DC.write_tree(tmp, opt, "train", [("0", anns, (w, h)), ("1", pre, (w, h))], tracking=True)
        opt.data_dir = tmp
        ds = M.ObjectPoseDataset(opt, "train")
        np.random.seed(seed)
        sample = ds[0]
    assert sample["ptk_gen"][0] == 1.0 and sample["ptk_det_meta"].shape == (12,)
    assert list(sample["ptk_det_meta"][8:12]) == [500.0, 510.0, w / 2.0, h / 2.0]


# ---- discovery, fall-back, unreadable images, collate ----

def _tree(tmp_path, layout, c="chair", root="outf"):
    """layout: {split: {video: [frame ids]}} -> files; returns the opt."""
    from PIL import Image

    anns = PC.synth_annotations(np.random.default_rng(3), [(None, "pose")], 64, 48)
    for split, videos in layout.items():
        for video, frames in videos.items():
            d = tmp_path / root / ("%s_%s" % (c, split)) / video
            d.mkdir(parents=True)
            for fid in frames:
                Image.fromarray(np.full((48, 64, 3), 7, np.uint8), "RGB").save(str(d / ("%s.png" % fid)))
                (d / ("%s.json" % fid)).write_text(json.dumps(anns))
    return PC.make_opt(dict(c=c, data_dir=str(tmp_path), data_generation_mode_ratio=0, flip=0.0, input_res=64, output_res=16))


def test_discovery_and_video_index(tmp_path):
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset

    opt = _tree(tmp_path, {"train": {"batch-1_3": ["00000", "00001"], "batch-2_0": ["00004"]}})
    (tmp_path / "outf" / "chair_train" / "batch-2_0" / "00009.png").write_bytes(b"no annotation beside it")
    ds = ObjectPoseDataset(opt, "train")
    assert len(ds) == 3 and ds.max_objs == 10 and ds.num_classes == 1 and ds.num_joints == 8
    assert sorted(ds.videos) == ["batch-1_3", "batch-2_0"] and len(ds.videos["batch-1_3"]) == 2
    for img, video, frame, ann in ds.images:
        assert os.path.basename(os.path.dirname(img)) == video and os.path.basename(img) == frame + ".png"
        assert ann == img[:-3] + "json" and os.path.exists(ann)
    # the reference's own walk: listdir order of the videos, glob order inside
    root = str(tmp_path / "outf" / "chair_train")
    order = [v for v in os.listdir(root)]
    assert [s[1] for s in ds.images] == [v for v in order for _ in ds.videos[v]]
    assert np.array_equal(ds._data_rng.get_state()[1], np.random.RandomState(123).get_state()[1])
    assert ds.flip_idx == [[1, 5], [3, 7], [2, 6], [4, 8]] and ds.mean.shape == (1, 1, 3) and ds.std.dtype == np.float32


def test_val_falls_back_to_test_split(tmp_path):
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset

    opt = _tree(tmp_path, {"train": {"v": ["0"]}, "test": {"v": ["0", "1"]}})
    val = ObjectPoseDataset(opt, "val")
    assert val.img_dir.endswith("chair_test") and len(val) == 2
    before = np.random.get_state()[1].copy()
    sample = val[0]
    assert np.array_equal(np.random.get_state()[1], before)  # no draws on val
    assert sample["frame"].shape == (48, 64, 3) and int(sample["frame"][0, 0, 0]) == 7
    (tmp_path / "outf" / "chair_val" / "v").mkdir(parents=True)
    assert ObjectPoseDataset(opt, "val").img_dir.endswith("chair_val")


def test_tracking_reads_outf_all(tmp_path):
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset

    opt = _tree(tmp_path, {"train": {"v": ["0"]}}, root="outf_all")
    opt.tracking_task = True
    assert len(ObjectPoseDataset(opt, "train")) == 1
    opt.tracking_task = False
    assert len(ObjectPoseDataset(opt, "train")) == 0


def test_unreadable_image_is_none_and_collate(tmp_path):
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset
    from centerpose_amd.lib.datasets.dataset_factory import collate_fn_filtered
    from PIL import Image

    opt = _tree(tmp_path, {"train": {"v": ["0", "1", "2"]}})
    d = tmp_path / "outf" / "chair_train" / "v"
    (d / "1.png").write_bytes(b"not a png")
    Image.fromarray(np.zeros((64, 48, 3), np.uint8), "RGB").save(str(d / "2.png"))  # portrait among landscape
    ds = ObjectPoseDataset(opt, "train")
    by_frame = {s[2]: i for i, s in enumerate(ds.images)}
    samples = {f: ds[i] for f, i in by_frame.items()}
    assert samples["1"] is None and samples["0"] is not None
    batch = collate_fn_filtered([samples["0"], samples["1"], samples["2"]])
    assert isinstance(batch["frame"], list) and [f.shape for f in batch["frame"]] == [(48, 64, 3), (64, 48, 3)]
    assert batch["frame"][0].dtype == np.uint8
    assert torch.is_tensor(batch["ti_image"]) and batch["ti_image"].shape == (2, 24) and batch["ti_image"].dtype == torch.float64
    assert batch["pt_objects"].shape == (2, 10, 64) and batch["pt_image"].shape == (2, 32)
    assert collate_fn_filtered([None, None]) is None and collate_fn_filtered([]) is None


def test_new_data_augmentation_is_refused(tmp_path):
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset

    opt = _tree(tmp_path, {"train": {"v": ["0"]}})
    opt.new_data_augmentation = True
    with pytest.raises(NotImplementedError, match="new_data_augmentation"):
        ObjectPoseDataset(opt, "train")


def test_dataset_never_builds_a_detector(tmp_path):
    """data_generation_mode_ratio > 0 constructs nothing here: the detector is the trainer's."""
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset

    opt = _tree(tmp_path, {"train": {"v": ["0"]}}, root="outf_all")
    opt.tracking_task, opt.data_generation_mode_ratio = True, 0.3
    ds = ObjectPoseDataset(opt, "train")
    assert not [a for a in vars(ds) if "detector" in a]
