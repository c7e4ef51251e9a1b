"""Device ``Smeasure`` / ``Emeasure`` / ``Fmeasure`` / ``WeightedFmeasure`` evaluators (twig/metric/{S,E,F}measure.py and
WeightedFmeasure.py around py_sod_metrics 1.3.1), opt-in with ``build_evaluators(..., sod_metrics="device")`` or ``val_cfg: {sod_metrics: device}``.

Wrapper semantics kept: ``process()`` steps every image of the batch, then appends ONE running value - the package's
``get_results()`` over every image seen so far: ``sm`` for S, ``em.curve.max()`` for E, ``fm.curve.max()`` for F, ``wfm`` for the weighted F - and
``compute_metrics()`` returns the mean of those per-batch values.  The arithmetic is csrc/sod_metrics.hip and, for the weighted F-measure, csrc/wfm.hip
(see runner/metrics.py for what is pinned).  Difference from the reference: state is reset at every ``Runner.validate()`` (``reset()``), where a persistent
mmengine metric object keeps stepping its py_sod_metrics evaluator across validation passes (with ``val_interval == max_epochs``
in both configs the reference validates once, so the figures agree there).

The evaluators built for one Runner share one ``SodAccumulator``: the kernel chain runs once per batch however many of the three
are configured, ``process()`` never synchronises, and the running values go to a growable device buffer that ``compute_metrics()``
reads once.  ``WeightedFmeasure`` runs its own chain and keeps its own two-entry state; when it is configured, ``summary()`` gains
``wFmeasure``.

``score_size: original`` (runner/config.py): ``process()`` receives an ``ops.RaggedMaps`` - the packed prediction bytes of
``ops.predict_maps`` and the packed GT planes, each image at its own size - instead of ``(pred, gt)`` at the network size, and the
shared accumulator runs ``dgtd_sod_metrics_ragged`` in place of ``dgtd_sod_metrics``; everything behind the rows is the same.  ``MAE``
is a device evaluator in that mode (below)."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import _lib as L
from ..ops.sod_metrics import STATE, RaggedMaps, sod_metrics_accumulate, sod_metrics_ragged_rows, sod_metrics_rows
from ..ops.wfm import WFM_STATE, weighted_fmeasure_accumulate, weighted_fmeasure_rows


class SodAccumulator:
    """Device state of the running get_results() of the evaluators: ``state`` (DGTD_SODM_STATE fp64) and one row
    (sm, max em, max fm, mae) per batch in ``running``; the last column is filled only when a device ``MAE`` was built on this
    accumulator (``want_mae``)."""

    def __init__(self):
        self.state: Optional[torch.Tensor] = None
        self.running: Optional[torch.Tensor] = None
        self.calls = 0
        self._last = None
        self._host = None
        self.wfm: Optional["WeightedFmeasure"] = None      # set by a WeightedFmeasure evaluator built on this accumulator
        self.want_mae = False                              # set by a device MAE evaluator built on this accumulator

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()
        self.calls = 0
        self._last = None
        self._host = None

    def step(self, k: int, pred, gt: Optional[torch.Tensor] = None) -> int:
        """Call ``k`` of one evaluator: the first evaluator to reach a batch runs the kernel chain for it; the others find the same
        (pred, gt) and reuse its slot.  ``pred`` is the prediction at the network size with its ``gt``, or an ``ops.RaggedMaps`` (each
        image at its own size, ``gt`` unused): the rows come from ``dgtd_sod_metrics`` or ``dgtd_sod_metrics_ragged``."""
        ragged = pred if isinstance(pred, RaggedMaps) else None
        if ragged is not None:
            pred, gt = ragged.pred8, ragged.gt8
        if k == self.calls - 1 and self._last is not None and self._last[0] is pred and self._last[1] is gt:
            return k
        if k != self.calls:
            raise L.DgtdError("evaluators that share one SodAccumulator must process the same batches in the same order")
        if self.state is None or self.state.device != pred.device:
            self.state = torch.zeros(STATE, dtype=torch.float64, device=pred.device)
            self.running = torch.empty(16, 4, dtype=torch.float64, device=pred.device)
        if k == self.running.shape[0]:
            grown = torch.empty(2 * k, 4, dtype=torch.float64, device=pred.device)
            grown[:k].copy_(self.running)
            self.running = grown
        rows = sod_metrics_rows(pred, gt) if ragged is None else sod_metrics_ragged_rows(ragged)
        sod_metrics_accumulate(rows, self.state, self.running[k])
        if self.want_mae:                                  # MAE's running mean over every image so far: sum mae / n, on the device
            torch.div(self.state[2], self.state[0], out=self.running[k, 3])
        self.calls += 1
        self._last = (pred, gt)
        self._host = None
        return k

    def running_values(self) -> List[List[float]]:
        """[(sm, max em, max fm, mae)] per batch, read from the device once per set of batches."""
        if self._host is None:
            self._host = self.running[:self.calls].cpu().tolist() if self.calls else []
        return self._host

    def summary(self) -> Dict[str, float]:
        """The final table of the reference's evaluation script (twig/metric/Fmeasure.py:62-74, commented out) over every image seen
        since the last reset: Smeasure, MAE, adpEm, meanEm, maxEm, adpFm, meanFm, maxFm - and wFmeasure when a WeightedFmeasure
        evaluator was built on this accumulator."""
        out = {}
        if self.calls:
            s = self.state.cpu()
            n = float(s[0])
            em, fm = s[8:264] / n, s[264:520] / n
            out = {"Smeasure": float(s[1]) / n, "MAE": float(s[2]) / n, "adpEm": float(s[3]) / n, "meanEm": float(em.mean()),
                   "maxEm": float(em.max()), "adpFm": float(s[4]) / n, "meanFm": float(fm.mean()), "maxFm": float(fm.max())}
        if self.wfm is not None:
            out.update(self.wfm.mean())
        return out


class _DeviceSodMetric:
    name = "metric"
    column = 0

    def __init__(self, accumulator: Optional[SodAccumulator] = None, **_ignored):
        self.acc = accumulator if accumulator is not None else SodAccumulator()
        self.results: List[int] = []          # slot index of each process() call (Runner.validate clears the list)

    def reset(self) -> None:
        self.results.clear()
        self.acc.reset()

    def process(self, data_batch, data_samples) -> None:
        if isinstance(data_samples, RaggedMaps):
            self.results.append(self.acc.step(len(self.results), data_samples))
        else:
            pred, gt = data_samples
            self.results.append(self.acc.step(len(self.results), pred, gt))

    def compute_metrics(self) -> Dict[str, float]:
        vals = self.acc.running_values()
        per_batch = [vals[i][self.column] for i in self.results]
        return {self.name: sum(per_batch) / max(1, len(per_batch))}

    def summary(self) -> Dict[str, float]:
        return self.acc.summary()


class Smeasure(_DeviceSodMetric):
    name, column = "Smeasure", 0


class Emeasure(_DeviceSodMetric):
    name, column = "Emeasure", 1


class Fmeasure(_DeviceSodMetric):
    name, column = "Fmeasure", 2


class MAE(_DeviceSodMetric):
    """twig/metric/MAE.py on the shared accumulator, for ``score_size: original``: the wrapper's running mean over every image seen
    (``sum mae / n`` after each batch, on the device), one host read in ``compute_metrics()``."""
    name, column = "MAE", 3

    def __init__(self, accumulator: Optional[SodAccumulator] = None, **_ignored):
        super().__init__(accumulator)
        self.acc.want_mae = True


class WeightedFmeasure:
    """twig/metric/WeightedFmeasure.py on csrc/wfm.hip.  It keeps its own device state ({n, sum wfm} and one running value per
    batch) beside the shared accumulator, whose ``summary()`` it extends with ``wFmeasure``."""
    name = "WeightedFmeasure"

    def __init__(self, accumulator: Optional[SodAccumulator] = None, **_ignored):
        self.acc = accumulator if accumulator is not None else SodAccumulator()
        self.acc.wfm = self
        self.results: List[int] = []
        self.state: Optional[torch.Tensor] = None
        self.running: Optional[torch.Tensor] = None
        self._host = None

    def reset(self) -> None:
        self.results.clear()
        if self.state is not None:
            self.state.zero_()
        self._host = None

    def process(self, data_batch, data_samples) -> None:
        pred, gt = data_samples
        k = len(self.results)
        if self.state is None or self.state.device != pred.device:
            self.state = torch.zeros(WFM_STATE, dtype=torch.float64, device=pred.device)
            self.running = torch.empty(16, dtype=torch.float64, device=pred.device)
        if k == self.running.shape[0]:
            grown = torch.empty(2 * k, dtype=torch.float64, device=pred.device)
            grown[:k].copy_(self.running)
            self.running = grown
        weighted_fmeasure_accumulate(weighted_fmeasure_rows(pred, gt), self.state, self.running[k:k + 1])
        self.results.append(k)
        self._host = None

    def compute_metrics(self) -> Dict[str, float]:
        if self._host is None:
            self._host = self.running[:len(self.results)].cpu().tolist() if self.results else []
        per_batch = [self._host[i] for i in self.results]
        return {self.name: sum(per_batch) / max(1, len(per_batch))}

    def mean(self) -> Dict[str, float]:
        """{"wFmeasure": mean over every image seen since the last reset}."""
        if not self.results:
            return {}
        s = self.state.cpu()
        return {"wFmeasure": float(s[1]) / float(s[0])}

    def summary(self) -> Dict[str, float]:
        return self.acc.summary()


DEVICE_EVALUATORS = {"Smeasure": Smeasure, "Emeasure": Emeasure, "Fmeasure": Fmeasure, "WeightedFmeasure": WeightedFmeasure}
