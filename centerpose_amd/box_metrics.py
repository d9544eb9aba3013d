"""Objectron accuracy of detector output: the metric half of the reference evaluator's `Evaluator.evaluate` /
`finalize` (src/tools/objectron_eval/eval_image_official.py:329-532, :1171-1179, objectron/dataset/metrics_nvidia.py)
without TFRecords, OpenCV or the detector.

The geometry of every matched pair -- 3D IoU, ADD, ADD-S and viewpoint over the `num_symmetry` rotations of
evaluate_3d, and evaluate_2d's reprojection sweep -- runs on the device, one `cp_box_eval` launch per `evaluate` call
(centerpose_amd/csrc/box3d.hip).  Matching, ground-plane rescaling, the scale error and the confidence-ranked
HitMiss / AveragePrecision bookkeeping stay on the host in numpy float64, as upstream; the AP sort runs in float32 with
numpy's default argsort, because ties decide AP.

    ev = BoxEvaluator(num_symmetry=100)
    ev.evaluate([(ret['boxes'], label, plane, projection_matrix), ...])   # any number of calls
    res = ev.finalize()   # res['ap']['iou'] etc.: 21-bin AP arrays; res['mean_error_2d'] etc.

Not covered (out of scope): eval_MobilePose_postprocessing (Lift2DTo3D), eval_gt_scale (re-PnP), evaluate_rotation,
per-video multiprocessing, drawing and debug output.
"""
import numpy as np

MAX_PIXEL_ERROR = 0.1
MAX_AZIMUTH_ERROR = 30.
MAX_POLAR_ERROR = 20.
MAX_SCALE_ERROR = 2.
MAX_DISTANCE = 1.0
NUM_BINS = 21
METRICS = ("scale", "iou", "pixel", "azimuth", "polar", "add", "adds")
# (upper threshold, greater-is-better) of each metric's 21 thresholds (eval_image_official.py:145-152)
_THRESH = {"scale": (1., False), "iou": (1., True), "pixel": (MAX_PIXEL_ERROR, False),
           "azimuth": (MAX_AZIMUTH_ERROR, False), "polar": (MAX_POLAR_ERROR, False), "add": (MAX_DISTANCE, False),
           "adds": (MAX_DISTANCE, False)}


def _device_pair_metrics(pred3d, gt3d, pred2d, mo2c, proj, single, num_symmetry):
    from centerpose_amd import hip

    return hip.box_eval(pred3d, gt3d, pred2d, mo2c, proj, single, num_symmetry)


def compute_ap(recall, precision):
    """AveragePrecision.compute_ap: VOC-style integration of the monotone precision envelope"""
    recall = np.insert(recall, 0, [0.])
    recall = np.append(recall, [1.])
    precision = np.insert(precision, 0, [0.])
    precision = np.append(precision, [0.])
    mono = precision.copy()
    for i in range(len(mono) - 2, -1, -1):
        mono[i] = max(mono[i], mono[i + 1])
    ap = 0.0
    for i in range(1, len(recall)):
        if recall[i] != recall[i - 1]:
            ap += (recall[i] - recall[i - 1]) * mono[i]
    return ap


class BoxEvaluator(object):
    """num_symmetry: eval_num_symmetry (the reference's shell scripts pass 100 for symmetric categories);
    mug_symmetric False with a label's MugFlag_instance evaluates mugs at rotation 0 only; use_absolute_scale False
    rescales each matched prediction onto the ground plane (compute_scale).  pair_metrics(pred3d, gt3d, pred2d, mo2c,
    proj, single_rotation, num_symmetry) -> [N, 9] records of cp_box_eval's layout; the default is the device."""

    def __init__(self, num_symmetry=1, mug_symmetric=True, use_absolute_scale=False, vis_thresh=0.1, pair_metrics=None):
        if num_symmetry < 1:
            raise ValueError("num_symmetry must be >= 1")
        self.num_symmetry = int(num_symmetry)
        self.mug_symmetric = mug_symmetric
        self.use_absolute_scale = use_absolute_scale
        self.vis_thresh = vis_thresh
        self.pair_metrics = pair_metrics or _device_pair_metrics
        self.thresholds = {m: np.linspace(0.0, hi, num=NUM_BINS) for m, (hi, _) in _THRESH.items()}
        # per metric and threshold: one list per image of [hit, conf] / [miss, conf] rows (HitMiss / AveragePrecision)
        self.hit = {m: [[] for _ in range(NUM_BINS)] for m in METRICS}
        self.miss = {m: [[] for _ in range(NUM_BINS)] for m in METRICS}
        self.total_instances = 0.
        self.matched = 0
        self.sums = {"scale": 0., "pixel": 0., "iou": 0., "azimuth": 0., "polar": 0.}
        # matched pairs whose viewpoint is undefined (CP_BOX_FLAG_SINGULAR_RAY: a singular 4 x 4 ray solve, where the
        # reference falls back to pinv): NaN azimuth / polar errors, a miss at every threshold, and left out of the two
        # viewpoint means, which divide by the pairs that have one
        self.flagged = 0
        self.viewpoint_pairs = 0

    @staticmethod
    def _is_visible(point):
        return point[0] > 0 and point[0] < 1 and point[1] > 0 and point[1] < 1

    def match_box(self, box, instances, visibilities):
        """nearest annotation by the Frobenius distance of the 8 projected vertices; -1 below the visibility threshold"""
        norms = np.linalg.norm(instances[:, 1:, :] - box[1:, :], axis=(1, 2))
        i_min = np.argmin(norms)
        if visibilities[i_min] < self.vis_thresh:
            return -1
        return i_min

    @staticmethod
    def compute_scale(box, plane):
        """the factor that puts the box's 4 lowest vertices (along the plane normal) on the ground plane"""
        center, normal = plane
        vertex_dots = [np.dot(vertex, normal) for vertex in box[1:]]
        vertex_dots = np.sort(vertex_dots)
        center_dot = np.dot(center, normal)
        scales = center_dot / vertex_dots[:4]
        return np.mean(scales)

    @staticmethod
    def scale_error(relative_scale, instance):
        rs = relative_scale / relative_scale[1]
        inst = instance / instance[1]
        return np.sum(np.absolute(rs - inst) / inst)

    def evaluate(self, images):
        """images: iterable of (boxes, label, plane, projection_matrix) per frame.
        boxes: the detector's ret['boxes'] entries (point_2d [9,2], point_3d [9,3], relative_scale [3], point_2d_ori,
        result with 'score'); label: '2d_instance' [I,9,2], '3d_instance' [I,9,3], 'scale_instance' [I,3],
        'Mo2c_instance' [I,4,4], 'visibility' [I], optional 'MugFlag_instance' [I]; plane: (centre [3], normal [3])."""
        frames, pairs = [], []
        for boxes, label, plane, proj in images:
            inst2d = np.asarray(label["2d_instance"], np.float64)
            inst3d = np.asarray(label["3d_instance"], np.float64)
            vis = np.asarray(label["visibility"])
            mug = label.get("MugFlag_instance")
            num_instances = 0
            for instance, instance_3d, visibility in zip(inst2d, inst3d, vis):
                if visibility > self.vis_thresh and self._is_visible(instance[0]) and instance_3d[0, 2] < 0:
                    num_instances += 1
            if num_instances == 0:  # no negative examples in the evaluation
                continue
            rows = []
            for box in boxes:
                point_2d, point_3d, relative_scale, _, result = box[:5]
                point_2d = np.asarray(point_2d, np.float64)
                point_3d = np.asarray(point_3d, np.float64)
                index = self.match_box(point_2d, inst2d, vis)
                if index >= 0:
                    if not self.use_absolute_scale:
                        point_3d = point_3d * self.compute_scale(point_3d, plane)
                    single = (not self.mug_symmetric) and mug is not None and bool(mug[index])
                    rows.append((len(pairs), self.scale_error(np.asarray(relative_scale, np.float64),
                                                              np.asarray(label["scale_instance"][index], np.float64)),
                                 result["score"]))
                    pairs.append((point_3d, inst3d[index], point_2d, np.asarray(label["Mo2c_instance"][index]),
                                  np.asarray(proj, np.float64), single))
                else:
                    rows.append(None)
            frames.append((rows, len(inst2d)))
        rec = np.zeros((0, 9))
        if pairs:
            rec = np.asarray(self.pair_metrics(*[np.array([p[k] for p in pairs], np.float64) for k in range(5)],
                                               np.array([p[5] for p in pairs], np.int32), self.num_symmetry))
        if len(rec):
            from centerpose_amd import hip

            bad = (rec[:, 8].astype(np.int64) & (hip.BOX_FLAG_SINGULAR_MO2C | hip.BOX_FLAG_CLIP_OVERFLOW)) != 0
            if bad.any():  # nothing of this call is recorded: the reference raises on a singular Mo2c_instance
                raise ValueError("BoxEvaluator: %d matched pair(s) with a singular Mo2c_instance or an overflowing clip "
                                 "(flags %s)" % (int(bad.sum()), sorted(set(rec[bad, 8].astype(int).tolist()))))
        for rows, n_inst in frames:
            hm = {m: [[] for _ in range(NUM_BINS)] for m in METRICS}
            for row in rows:
                if row is None:
                    conf = 0
                    val = {"scale": MAX_SCALE_ERROR, "iou": 0., "add": MAX_DISTANCE, "adds": MAX_DISTANCE,
                           "pixel": MAX_PIXEL_ERROR, "azimuth": MAX_AZIMUTH_ERROR, "polar": MAX_POLAR_ERROR}
                else:
                    k, scale_err, conf = row
                    r = rec[k]
                    val = {"scale": scale_err, "iou": r[0], "add": r[1], "adds": r[2], "pixel": r[5], "azimuth": r[3],
                           "polar": r[4]}
                    self.matched += 1
                    for m in ("scale", "pixel", "iou"):
                        self.sums[m] += val[m]
                    if int(r[8]) & 1:  # CP_BOX_FLAG_SINGULAR_RAY
                        self.flagged += 1
                    else:
                        self.viewpoint_pairs += 1
                        self.sums["azimuth"] += val["azimuth"]
                        self.sums["polar"] += val["polar"]
                for m in METRICS:
                    greater = _THRESH[m][1]
                    for i, th in enumerate(self.thresholds[m]):
                        hit = (greater and val[m] >= th) or ((not greater) and val[m] <= th)
                        hm[m][i].append([1 if hit else 0, conf])
            for m in METRICS:
                for i in range(NUM_BINS):
                    self.hit[m][i].append(hm[m][i])
                    self.miss[m][i].append([[1 - h, c] for h, c in hm[m][i]])
            self.total_instances += n_inst
        return rec

    def hit_miss_arrays(self, metric):
        """[21, R, 2] hit and miss rows of every record so far, in evaluation order (HitMiss.hit / .miss, flattened)"""
        hit = np.array([[row for img in self.hit[metric][i] for row in img] for i in range(NUM_BINS)], np.float64)
        miss = np.array([[row for img in self.miss[metric][i] for row in img] for i in range(NUM_BINS)], np.float64)
        return hit.reshape(NUM_BINS, -1, 2), miss.reshape(NUM_BINS, -1, 2)

    def _ap(self, metric):
        if self.total_instances == 0:
            raise ValueError("No instances in the computation.")
        aps = np.zeros(NUM_BINS)
        for i in range(NUM_BINS):
            tp = [k for j in self.hit[metric][i] for k in j]
            fp = [k for j in self.miss[metric][i] for k in j]
            if len(fp) != 0 and len(tp) != 0:
                combined = np.concatenate((tp, fp), axis=1).astype('float32')
                combined = combined[np.argsort(-combined[:, 1])]
                tpc = np.cumsum(combined[:, 0])
                fpc = np.cumsum(combined[:, 2])
                tp_fp = tpc + fpc
                recall = tpc / self.total_instances
                precision = np.divide(tpc, tp_fp, out=np.zeros_like(tpc), where=tp_fp != 0)
                aps[i] = compute_ap(recall, precision)
        return aps

    def finalize(self):
        """{'ap': {metric: [21] AP}, 'thresholds': {metric: [21]}, 'mean_error_scale' / '_2d' / 'mean_iou_3d' /
        'mean_error_azimuth' / '_polar' (write_report's means over the matched pairs; the two viewpoint means over the
        matched pairs with a defined viewpoint), 'matched', 'flagged' (matched pairs without a viewpoint)}"""
        div = float(self.matched) if self.matched > 0 else 1e-6
        vdiv = float(self.viewpoint_pairs) if self.viewpoint_pairs > 0 else 1e-6
        return {"ap": {m: self._ap(m) for m in METRICS}, "thresholds": dict(self.thresholds),
                "mean_error_scale": self.sums["scale"] / div, "mean_error_2d": self.sums["pixel"] / div,
                "mean_iou_3d": self.sums["iou"] / div, "mean_error_azimuth": self.sums["azimuth"] / vdiv,
                "mean_error_polar": self.sums["polar"] / vdiv, "matched": self.matched, "flagged": self.flagged}
