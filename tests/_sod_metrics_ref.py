"""NumPy fp64 restatement of py_sod_metrics 1.3.1 (Smeasure, Emeasure, Fmeasure, MAE) and of the reference's wrappers around it
(twig/metric/{S,E,F}measure.py, MAE.py), written in the package's own operation order.  Test helper only: the package never imports
it.  The E-measure follows the reference's commented copy of the package code (twig/metric/Emeasure.py:51-243)."""
from __future__ import annotations

import numpy as np

EPS = np.spacing(1)
TYPE = np.float64


def quantise(x) -> np.ndarray:
    """wrapper: (x * 255).astype(np.uint8) on the fp32 map (fp32 multiply, truncating cast)."""
    x = np.asarray(x, dtype=np.float32)
    return (x * 255).astype(np.uint8)


def _prepare_data(pred: np.ndarray, gt: np.ndarray):
    gt = gt > 128
    pred = pred / 255
    if pred.max() != pred.min():
        pred = (pred - pred.min()) / (pred.max() - pred.min())
    return pred, gt


def _get_adaptive_threshold(matrix: np.ndarray, max_value: float = 1) -> float:
    return min(2 * matrix.mean(), max_value)


class Fmeasure:
    def __init__(self, beta: float = 0.3):
        self.beta = beta
        self.precisions, self.recalls, self.adaptive_fms, self.changeable_fms = [], [], [], []

    def step(self, pred, gt):
        pred, gt = _prepare_data(pred, gt)
        self.adaptive_fms.append(self.cal_adaptive_fm(pred, gt))
        precisions, recalls, changeable_fms = self.cal_pr(pred, gt)
        self.precisions.append(precisions)
        self.recalls.append(recalls)
        self.changeable_fms.append(changeable_fms)

    def cal_adaptive_fm(self, pred, gt):
        adaptive_threshold = _get_adaptive_threshold(pred, max_value=1)
        binary_predcition = pred >= adaptive_threshold
        area_intersection = binary_predcition[gt].sum()
        if area_intersection == 0:
            return 0
        pre = area_intersection / np.count_nonzero(binary_predcition)
        rec = area_intersection / np.count_nonzero(gt)
        return (1 + self.beta) * pre * rec / (self.beta * pre + rec)

    def cal_pr(self, pred, gt):
        pred = (pred * 255).astype(np.uint8)
        bins = np.linspace(0, 256, 257)
        fg_hist, _ = np.histogram(pred[gt], bins=bins)
        bg_hist, _ = np.histogram(pred[~gt], bins=bins)
        fg_w_thrs = np.cumsum(np.flip(fg_hist), axis=0)
        bg_w_thrs = np.cumsum(np.flip(bg_hist), axis=0)
        TPs = fg_w_thrs
        Ps = fg_w_thrs + bg_w_thrs
        Ps[Ps == 0] = 1
        T = max(np.count_nonzero(gt), 1)
        precisions = TPs / Ps
        recalls = TPs / T
        numerator = (1 + self.beta) * precisions * recalls
        denominator = np.where(numerator == 0, 1, self.beta * precisions + recalls)
        return precisions, recalls, numerator / denominator

    def get_results(self):
        return dict(fm=dict(adp=np.mean(np.array(self.adaptive_fms, TYPE)),
                            curve=np.mean(np.array(self.changeable_fms, dtype=TYPE), axis=0)),
                    pr=dict(p=np.mean(np.array(self.precisions, dtype=TYPE), axis=0),
                            r=np.mean(np.array(self.recalls, dtype=TYPE), axis=0)))


class MAE:
    def __init__(self):
        self.maes = []

    def step(self, pred, gt):
        pred, gt = _prepare_data(pred, gt)
        self.maes.append(np.mean(np.abs(pred - gt)))

    def get_results(self):
        return dict(mae=np.mean(np.array(self.maes, TYPE)))


class Smeasure:
    def __init__(self, alpha: float = 0.5):
        self.sms = []
        self.alpha = alpha

    def step(self, pred, gt):
        pred, gt = _prepare_data(pred=pred, gt=gt)
        self.sms.append(self.cal_sm(pred, gt))

    def cal_sm(self, pred, gt):
        y = np.mean(gt)
        if y == 0:
            sm = 1 - np.mean(pred)
        elif y == 1:
            sm = np.mean(pred)
        else:
            sm = self.alpha * self.object(pred, gt) + (1 - self.alpha) * self.region(pred, gt)
            sm = max(0, sm)
        return sm

    def object(self, pred, gt):
        fg = pred * gt
        bg = (1 - pred) * (1 - gt)
        u = np.mean(gt)
        return u * self.s_object(fg, gt) + (1 - u) * self.s_object(bg, 1 - gt)

    def s_object(self, pred, gt):
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.mean(pred[gt == 1])
            sigma_x = np.std(pred[gt == 1], ddof=1)
        return 2 * x / (np.power(x, 2) + 1 + sigma_x + EPS)

    def region(self, pred, gt):
        x, y = self.centroid(gt)
        part_info = self.divide_with_xy(pred, gt, x, y)
        w1, w2, w3, w4 = part_info["weight"]
        pred1, pred2, pred3, pred4 = part_info["pred"]
        gt1, gt2, gt3, gt4 = part_info["gt"]
        return (w1 * self.ssim(pred1, gt1) + w2 * self.ssim(pred2, gt2) + w3 * self.ssim(pred3, gt3)
                + w4 * self.ssim(pred4, gt4))

    def centroid(self, matrix):
        h, w = matrix.shape
        if np.count_nonzero(matrix) == 0:
            x, y = np.round(w / 2), np.round(h / 2)
        else:
            y, x = np.argwhere(matrix).mean(axis=0).round()
        return int(x) + 1, int(y) + 1

    def divide_with_xy(self, pred, gt, x, y):
        h, w = gt.shape
        area = h * w
        w1 = x * y / area
        w2 = y * (w - x) / area
        w3 = (h - y) * x / area
        w4 = 1 - w1 - w2 - w3
        return dict(gt=(gt[0:y, 0:x], gt[0:y, x:w], gt[y:h, 0:x], gt[y:h, x:w]),
                    pred=(pred[0:y, 0:x], pred[0:y, x:w], pred[y:h, 0:x], pred[y:h, x:w]),
                    weight=(w1, w2, w3, w4))

    def ssim(self, pred, gt):
        h, w = pred.shape
        N = h * w
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.mean(pred)
            y = np.mean(gt)
            sigma_x = np.sum((pred - x) ** 2) / (N - 1)
            sigma_y = np.sum((gt - y) ** 2) / (N - 1)
            sigma_xy = np.sum((pred - x) * (gt - y)) / (N - 1)
            alpha = 4 * x * y * sigma_xy
            beta = (x ** 2 + y ** 2) * (sigma_x + sigma_y)
            if alpha != 0:
                return alpha / (beta + EPS)
            if alpha == 0 and beta == 0:
                return 1
            return 0

    def get_results(self):
        return dict(sm=np.mean(np.array(self.sms, dtype=TYPE)))


class Emeasure:
    def __init__(self):
        self.adaptive_ems, self.changeable_ems = [], []

    def step(self, pred, gt):
        pred, gt = _prepare_data(pred=pred, gt=gt)
        self.gt_fg_numel = np.count_nonzero(gt)
        self.gt_size = gt.shape[0] * gt.shape[1]
        self.changeable_ems.append(self.cal_em_with_cumsumhistogram(pred, gt))
        self.adaptive_ems.append(self.cal_em_with_threshold(pred, gt, _get_adaptive_threshold(pred, max_value=1)))

    def cal_em_with_threshold(self, pred, gt, threshold):
        binarized_pred = pred >= threshold
        fg_fg_numel = np.count_nonzero(binarized_pred & gt)
        fg_bg_numel = np.count_nonzero(binarized_pred & ~gt)
        fg___numel = fg_fg_numel + fg_bg_numel
        bg___numel = self.gt_size - fg___numel
        if self.gt_fg_numel == 0:
            enhanced_matrix_sum = bg___numel
        elif self.gt_fg_numel == self.gt_size:
            enhanced_matrix_sum = fg___numel
        else:
            parts_numel, combinations = self.generate_parts_numel_combinations(fg_fg_numel, fg_bg_numel, fg___numel, bg___numel)
            results_parts = []
            for part_numel, combination in zip(parts_numel, combinations):
                align_matrix_value = 2 * (combination[0] * combination[1]) / (combination[0] ** 2 + combination[1] ** 2 + EPS)
                enhanced_matrix_value = (align_matrix_value + 1) ** 2 / 4
                results_parts.append(enhanced_matrix_value * part_numel)
            enhanced_matrix_sum = sum(results_parts)
        return enhanced_matrix_sum / (self.gt_size - 1 + EPS)

    def cal_em_with_cumsumhistogram(self, pred, gt):
        pred = (pred * 255).astype(np.uint8)
        bins = np.linspace(0, 256, 257)
        fg_fg_hist, _ = np.histogram(pred[gt], bins=bins)
        fg_bg_hist, _ = np.histogram(pred[~gt], bins=bins)
        fg_fg_numel_w_thrs = np.cumsum(np.flip(fg_fg_hist), axis=0)
        fg_bg_numel_w_thrs = np.cumsum(np.flip(fg_bg_hist), axis=0)
        fg___numel_w_thrs = fg_fg_numel_w_thrs + fg_bg_numel_w_thrs
        bg___numel_w_thrs = self.gt_size - fg___numel_w_thrs
        if self.gt_fg_numel == 0:
            enhanced_matrix_sum = bg___numel_w_thrs
        elif self.gt_fg_numel == self.gt_size:
            enhanced_matrix_sum = fg___numel_w_thrs
        else:
            parts_numel_w_thrs, combinations = self.generate_parts_numel_combinations(
                fg_fg_numel_w_thrs, fg_bg_numel_w_thrs, fg___numel_w_thrs, bg___numel_w_thrs)
            results_parts = np.empty(shape=(4, 256), dtype=np.float64)
            for i, (part_numel, combination) in enumerate(zip(parts_numel_w_thrs, combinations)):
                align_matrix_value = 2 * (combination[0] * combination[1]) / (combination[0] ** 2 + combination[1] ** 2 + EPS)
                enhanced_matrix_value = (align_matrix_value + 1) ** 2 / 4
                results_parts[i] = enhanced_matrix_value * part_numel
            enhanced_matrix_sum = results_parts.sum(axis=0)
        return enhanced_matrix_sum / (self.gt_size - 1 + EPS)

    def generate_parts_numel_combinations(self, fg_fg_numel, fg_bg_numel, pred_fg_numel, pred_bg_numel):
        bg_fg_numel = self.gt_fg_numel - fg_fg_numel
        bg_bg_numel = pred_bg_numel - bg_fg_numel
        parts_numel = [fg_fg_numel, fg_bg_numel, bg_fg_numel, bg_bg_numel]
        mean_pred_value = pred_fg_numel / self.gt_size
        mean_gt_value = self.gt_fg_numel / self.gt_size
        demeaned_pred_fg_value = 1 - mean_pred_value
        demeaned_pred_bg_value = 0 - mean_pred_value
        demeaned_gt_fg_value = 1 - mean_gt_value
        demeaned_gt_bg_value = 0 - mean_gt_value
        combinations = [(demeaned_pred_fg_value, demeaned_gt_fg_value), (demeaned_pred_fg_value, demeaned_gt_bg_value),
                        (demeaned_pred_bg_value, demeaned_gt_fg_value), (demeaned_pred_bg_value, demeaned_gt_bg_value)]
        return parts_numel, combinations

    def get_results(self):
        return dict(em=dict(adp=np.mean(np.array(self.adaptive_ems, dtype=TYPE)),
                            curve=np.mean(np.array(self.changeable_ems, dtype=TYPE), axis=0)))


def per_image(pred_f32, gt_f32) -> dict:
    """Every per-image quantity the device op returns, for one [H,W] pair of fp32 maps."""
    p8, g8 = quantise(pred_f32), quantise(gt_f32)
    S, E, F, M = Smeasure(), Emeasure(), Fmeasure(), MAE()
    for m in (S, E, F, M):
        m.step(p8, g8)
    return dict(mae=float(M.maes[0]), sm=float(S.sms[0]), adp_em=float(E.adaptive_ems[0]), adp_fm=float(F.adaptive_fms[0]),
                em_curve=np.asarray(E.changeable_ems[0], TYPE), fm_curve=F.changeable_fms[0], precision=F.precisions[0],
                recall=F.recalls[0])


def square_is_pow(gt_f32) -> bool:
    """True when the package's Python-float ``x ** 2`` of the two demeaned gt values equals ``x * x`` for this image (the E-measure
    curve is then bit-identical to a kernel that multiplies)."""
    g = quantise(gt_f32) > 128
    n, c = g.size, int(np.count_nonzero(g))
    if c in (0, n):
        return True
    vals = (1 - c / n, 0 - c / n)
    return all(v ** 2 == v * v for v in vals)


class Wrappers:
    """The reference's S/E/F/MAE wrappers: one running value appended per batch, compute_metrics = mean of those values."""

    def __init__(self):
        self.S, self.E, self.F, self.M = Smeasure(), Emeasure(), Fmeasure(), MAE()
        self.results = {"Smeasure": [], "Emeasure": [], "Fmeasure": [], "MAE": []}

    def process(self, pred_b, gt_b):
        for x, y in zip(np.asarray(pred_b, np.float32).reshape(len(pred_b), *np.shape(pred_b)[-2:]),
                        np.asarray(gt_b, np.float32).reshape(len(gt_b), *np.shape(gt_b)[-2:])):
            p8, g8 = quantise(x), quantise(y)
            for m in (self.S, self.E, self.F, self.M):
                m.step(p8, g8)
        self.results["Smeasure"].append(self.S.get_results()["sm"])
        self.results["Emeasure"].append(self.E.get_results()["em"]["curve"].max())
        self.results["Fmeasure"].append(self.F.get_results()["fm"]["curve"].max())
        self.results["MAE"].append(self.M.get_results()["mae"])

    def compute_metrics(self) -> dict:
        return {k: float(sum(v) / len(v)) for k, v in self.results.items()}

    def summary(self) -> dict:
        fm, em = self.F.get_results()["fm"], self.E.get_results()["em"]
        return {"Smeasure": float(self.S.get_results()["sm"]), "MAE": float(self.M.get_results()["mae"]), "adpEm": float(em["adp"]),
                "meanEm": float(em["curve"].mean()), "maxEm": float(em["curve"].max()), "adpFm": float(fm["adp"]),
                "meanFm": float(fm["curve"].mean()), "maxFm": float(fm["curve"].max())}
