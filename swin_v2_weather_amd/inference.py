"""Registry checkpoints and autoregressive inference on the HIP model.

The reference publishes its models as registry folders (README.md:32-44)

    swin_73var_depth12_chweight_invar/{hyperparams.yaml, weights.tar, global_means.npy, global_stds.npy, metadata.json}

where `hyperparams.yaml` is the flat dump of the training `params` (train.py:156-163) and `weights.tar` is the training
checkpoint (train.py:374-378): `{'model_state': state_dict, ...}` saved from the DDP-wrapped wrapper, i.e. keys
`module.model.<swin key>`.  `load_registry_model` builds the model of that yaml behind the same `get_model` surface and
loads the weights with any of the prefixes the reference produces (`module.model.`, `model.`, none);
`rollout` is the inference loop of MultiStepWrapper (helpers.py:26-41) for an arbitrary number of steps without autograd:
prediction fed back, next cos-zenith channel and the invariant channels re-appended.

`score_rollout` is the same loop with every step scored against the verifying analysis as soon as it is written
(utils/weighted_acc_rmse.ForecastScorer: latitude-weighted RMSE and ACC per channel and lead time, one pass per step; with
extremes=True also the top-quantile error, ForecastScorer.quantile_error; with spectrum=True also the spherical-harmonic degree power
of forecast and analysis, ForecastScorer.power_spectrum, and the small-scale power ratio that shows a rollout blurring).

`ensemble_rollout` perturbs the initial condition (`perturb_initial_condition`: member 0 is the unperturbed control), rolls the M
members out in the same loop and scores every step as an ensemble (ForecastScorer.ensemble_score: CRPS, fair CRPS, spread,
ensemble-mean RMSE and the rank histogram per channel and lead time, one pass over the members per step).

    python -m swin_v2_weather_amd.inference --registry DIR --steps 8 [--init x0.npy] [--out forecast.npy]
                                            [--truth truth.npy [--climatology time_means.npy] [--scores-out scores.json] [--extremes]
                                             [--score-grid DEG]
                                             [--spectrum] [--spectrum-out spectrum.npz] [--coherence]
                                             [--event-anomaly S [S ...] | --event-quantile Q [Q ...]] [--event-below] [--event-scales R [R ...]]
                                             [--ensemble M --perturbation A [--seed S] [--member-batch K] [--perturbation-scale KM]
                                              [--ensemble-scales R [R ...] [--ensemble-member-scores]]]]
"""
from __future__ import annotations

import argparse
import json
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from .networks.helpers import get_model
from .utils.YParams import load_yaml
from .utils.regrid import Regridder, grid_for_degrees, model_grid
from .utils.sht import coherence_scale
from .utils.weighted_acc_rmse import (EventSpec, ForecastScorer, RegriddedScorer, load_climatology, small_scale_power_ratio,  # noqa: F401
                                      spread_skill_ratio)


class _Params(dict):
    """flat hyperparams.yaml -> the attribute + item access train.py's `params` offers"""
    __getattr__ = dict.__getitem__

    def __contains__(self, k):
        return dict.__contains__(self, k)


def load_hyperparams(path) -> _Params:
    hp = load_yaml(path)
    if not isinstance(hp, dict):
        raise ValueError(f"{path}: expected a flat mapping of hyper-parameters")
    p = _Params({k: (None if v == 'None' else v) for k, v in hp.items()})
    p.setdefault("nettype", "swin")
    if "n_in_channels" not in p:                      # derived in train.py:88-98, dumped with the rest when training ran
        n = len(p["in_channels"])
        p["n_in_channels"] = n + int(bool(p.get("add_zenith", False))) + 2 * int(bool(p.get("add_landmask", False))) + \
            int(bool(p.get("add_orography", False)))
        p["n_out_channels"] = len(p["out_channels"])
    for k, d in (("activation_ckpt", False), ("residual", False), ("add_orography", False), ("add_landmask", False),
                 ("add_zenith", False), ("mlp_ratio", 4), ("full_pos_embed", True), ("rel_pos", False), ("drop_path_rate", 0.0)):
        p.setdefault(k, d)
    return p


def load_model_state(model: torch.nn.Module, state: dict) -> None:
    """load a reference state_dict whatever wrapper prefixes it carries (train.py:381-389 strips 'module.' by position)"""
    want = set(model.state_dict().keys())
    for strip in ("", "module.", "module.model.", "model."):
        cand = {(k[len(strip):] if k.startswith(strip) else k): v for k, v in state.items()}
        for add in ("", "model."):
            cand2 = {add + k: v for k, v in cand.items()}
            if set(cand2.keys()) == want:
                model.load_state_dict(cand2, strict=True)
                return
    missing = sorted(want - set(state.keys()))[:5]
    raise KeyError(f"checkpoint keys do not match the model under any known prefix (first missing: {missing})")


def load_registry_model(model_dir: str, device="cuda:0", trust_checkpoint: bool = False):
    """-> (single-step model in eval mode on `device`, params, (means, stds) or None).
    `weights.tar` is a published / third-party file: it is read with torch's restricted unpickler (tensors, state dicts and
    plain containers only).  trust_checkpoint=True falls back to the full unpickler -- arbitrary code execution from the file --
    for checkpoints that carry other objects; only for files you produced yourself."""
    p = load_hyperparams(os.path.join(model_dir, "hyperparams.yaml"))
    p["n_future"] = 0
    model = get_model(p)
    ck = torch.load(os.path.join(model_dir, "weights.tar"), map_location="cpu", weights_only=not trust_checkpoint)
    load_model_state(model, ck["model_state"] if "model_state" in ck else ck)
    stats = None
    gm, gs = os.path.join(model_dir, "global_means.npy"), os.path.join(model_dir, "global_stds.npy")
    if os.path.isfile(gm) and os.path.isfile(gs):
        stats = (np.load(gm), np.load(gs))
    return model.to(device).eval(), p, stats


def _rollout_steps(net, x0, n_steps, coszen, n_invar, out, coff_of):
    """the autoregressive loop: step s writes its prediction into out[:, coff_of(s) : coff_of(s) + Cout]; yields s after each step"""
    B, _, H, W = x0.shape
    invars = x0[:, x0.shape[1] - n_invar:] if n_invar else None
    x = x0
    for s in range(n_steps):
        extra = None
        if s + 1 < n_steps:
            parts = ([coszen[:, s:s + 1]] if coszen is not None else []) + ([invars] if n_invar else [])
            extra = torch.cat(parts, 1).float() if parts else x0.new_empty(B, 0, H, W)
        _, x = net.forward_rollout(x, out, coff_of(s), extra)
        yield s


def _ring(rows, n_steps, Cout, H, W, device, keep_forecast):
    """-> (out [rows, slots Cout, H, W]: a slot per step if keep_forecast, else a ring of two; coff_of: s -> step s's first channel; forecast)"""
    out = torch.empty(rows, (n_steps if keep_forecast else 2) * Cout, H, W, dtype=torch.float32, device=device)
    return out, (lambda s: (s if keep_forecast else s % 2) * Cout), out.view(rows, n_steps, Cout, H, W) if keep_forecast else None


@torch.no_grad()
def rollout(model, x0: torch.Tensor, n_steps: int, coszen: torch.Tensor | None = None, n_invar: int = 0) -> torch.Tensor:
    """x0 [B, Cin, H, W] (fields | zenith(t0) | invariants) -> forecasts [B, n_steps, Cout, H, W].
    coszen [B, n_steps - 1, H, W]: cos-zenith of the steps 1 .. n_steps - 1 inputs (required iff the model takes one)."""
    net = model.model if hasattr(model, "model") else model
    B, _, H, W = x0.shape
    out, coff_of, forecast = _ring(B, n_steps, net.out_chans, H, W, x0.device, True)
    for _ in _rollout_steps(net, x0, n_steps, coszen, n_invar, out, coff_of):
        pass
    return forecast


# degree power of forecast and analysis per lead time (batch means [n_steps, Cout, lmax]) and small_scale_power_ratio [n_steps, B, Cout]
RolloutSpectrum = namedtuple("RolloutSpectrum", "pred truth ratio")
# spectral coherence of forecast against analysis per lead time: the batch mean [n_steps, Cout, lmax] (fp64; NaN where a power is zero), the
# effective resolution coherence_scale(., level) per sample [n_steps, B, Cout] (int64) and the level it was taken at
RolloutCoherence = namedtuple("RolloutCoherence", "coherence scale level")
COHERENCE_LEVEL = 0.5
# events=EventSpec(kind, levels, below) of score_rollout: per lead time the thresholds used ([K] for "anomaly", [B, C, K] for "quantile"), the
# tables [n_steps, B, C, K, 4], n_invalid [n_steps, B, C] and `scores`: name -> [n_steps, C, K] fp64, from the tables summed over the batch
RolloutEvents = namedtuple("RolloutEvents", "spec thresholds table n_invalid scores")
# the same of ensemble_rollout: sums [n_steps, B, C, K, 3], wv [n_steps, B, C], hist [n_steps, B, C, K, 2, M + 1], n_invalid, and `scores`:
# brier, fair_brier, brier_skill, reliability, resolution, uncertainty, roc_area -> [n_steps, C, K] fp64, pooled over the batch
EnsembleRolloutEvents = namedtuple("EnsembleRolloutEvents", "spec thresholds sums wv hist n_invalid scores")
# neighbourhoods=(r, ...) of score_rollout, beside events=: the scales as given, rows [n_steps, B, C, K, S, H, 3] int64, n_invalid
# [n_steps, B, C] and `scores`: fss, fbs [n_steps, C, K, S], fss_uniform, base_rate, useful_scale [n_steps, C, K], from the rows summed over
# the batch (utils/events.py::fss_scores)
RolloutNeighbourhoods = namedtuple("RolloutNeighbourhoods", "scales rows n_invalid scores")
# ensemble_neighbourhoods=(r, ...) of ensemble_rollout, beside events=: the scales as given, rows [n_steps, B, C, K, S, H, 3] int64 of
# swv2_fss_ens_rows, n_invalid [n_steps, B, C] and `scores`: pfss, fbs [n_steps, C, K, S], fss_uniform, base_rate, useful_scale
# [n_steps, C, K], from the rows summed over the batch (utils/events.py::fss_ens_scores).  With member_neighbourhoods also member_rows and
# dispersion_rows [n_steps, B, C, K, S, H, 3] and member_scores / dispersion_scores (fss = eFSS / dFSS, ...), else None
EnsembleRolloutNeighbourhoods = namedtuple("EnsembleRolloutNeighbourhoods", "scales rows n_invalid scores member_rows dispersion_rows member_scores "
                                           "dispersion_scores", defaults=(None, None, None, None))


def _stack_scores(per_step):
    """[{name: [C, K]} per step] -> {name: [n_steps, C, K]}"""
    return {k: torch.stack([d[k] for d in per_step], dim=0) for k in per_step[0]}


class RolloutScores(namedtuple("RolloutScores", "rmse acc rmse_samples acc_samples forecast tqe", defaults=(None,))):
    """score_rollout's answer.  The tuple keeps its six fields (callers unpack and build it positionally); `spectrum` rides along as an
    attribute: None, or the RolloutSpectrum of score_rollout(..., spectrum=True); so does `events`: None, or the RolloutEvents of
    score_rollout(..., events=spec), and `neighbourhoods`: None, or the RolloutNeighbourhoods of score_rollout(..., events=spec,
    neighbourhoods=scales), and `coherence`: None, or the RolloutCoherence of score_rollout(..., coherence=True).  (_replace builds a new
    tuple: carry them over by hand.)"""
    spectrum = None
    coherence = None
    events = None
    neighbourhoods = None

    def with_spectrum(self, spectrum):
        self.spectrum = spectrum
        return self


def _truth_at(truth, s, device):
    return (truth(s) if callable(truth) else truth[:, s]).to(device)


def _check_events(who, events, scorer, neighbourhoods=None):
    if events is not None and events.kind == "anomaly" and scorer.clim is None:
        raise ValueError(f"{who}: anomaly events need a scorer with a climatology")
    if neighbourhoods is not None and events is None:
        raise ValueError(f"{who}: neighbourhoods are taken around the events of events=: give an EventSpec")


class _StepScores:
    """the per-step results of ONE deterministic forecast: score_rollout's, and the control (member 0) of ensemble_rollout"""

    def __init__(self, scorer, n_steps, B, Cout, H, device, events=None, extremes=False, spectrum=False, neighbourhoods=None, coherence=False):
        new = lambda *shape: torch.empty(n_steps, *shape, dtype=torch.float32, device=device)      # noqa: E731
        self.rmse, self.rmse_s = new(Cout), new(B, Cout)
        self.acc, self.acc_s = (new(Cout), new(B, Cout)) if scorer.clim is not None else (None, None)
        self.tqe = new(B, Cout) if extremes else None
        self.spec = RolloutSpectrum(new(Cout, H), new(Cout, H), new(B, Cout)) if spectrum else None
        self.coh = RolloutCoherence(torch.empty(n_steps, Cout, H, dtype=torch.float64, device=device),
                                    torch.empty(n_steps, B, Cout, dtype=torch.int64, device=device), COHERENCE_LEVEL) if coherence else None
        self.events, self.ev = events, []
        self.scales, self.nb = (None if neighbourhoods is None else tuple(neighbourhoods)), []

    def add(self, s, scorer, out, tar, coff):
        r = scorer.score(out, tar, coff_prd=coff)
        if self.tqe is not None:
            self.tqe[s] = scorer.quantile_error(out, tar, coff_prd=coff)
        if self.spec is not None:
            ps = scorer.power_spectrum(out, tar, coff_prd=coff)
            self.spec.pred[s], self.spec.truth[s], self.spec.ratio[s] = ps.pred.mean(dim=0), ps.truth.mean(dim=0), small_scale_power_ratio(ps.pred, ps.truth)
        if self.coh is not None:
            coh = scorer.spectral_coherence(out, tar, coff_prd=coff)
            self.coh.coherence[s], self.coh.scale[s] = coh.mean(dim=0), coherence_scale(coh, self.coh.level)
        self.rmse[s], self.rmse_s[s] = r.rmse_mean, r.rmse
        if self.acc is not None:
            self.acc[s], self.acc_s[s] = r.acc_mean, r.acc

    def add_events(self, s, scorer, out, tar, coff, thr=None):      # (a call of its own: the control scores its events first, on the ensemble's thr)
        if self.events is not None:
            thr = scorer.event_thresholds(self.events, tar) if thr is None else thr
            self.ev.append((thr, scorer.event_score(out, tar, thr, anomaly=self.events.kind == "anomaly", below=self.events.below, coff_prd=coff)))
            if self.scales is not None:
                self.nb.append(scorer.neighbourhood_score(out, tar, thr, self.scales, anomaly=self.events.kind == "anomaly", below=self.events.below,
                                                          coff_prd=coff))

    def result(self, forecast) -> RolloutScores:
        res = RolloutScores(self.rmse, self.acc, self.rmse_s, self.acc_s, forecast, self.tqe).with_spectrum(self.spec)
        res.coherence = self.coh
        if self.events is not None:           # the EventScores of every step -> RolloutEvents
            res.events = RolloutEvents(self.events, [t for t, _ in self.ev], torch.stack([e.table for _, e in self.ev], dim=0),
                                       torch.stack([e.n_invalid for _, e in self.ev], dim=0), _stack_scores([e.pooled for _, e in self.ev]))
        if self.scales is not None:
            res.neighbourhoods = RolloutNeighbourhoods(self.scales, torch.stack([n.rows for n in self.nb], dim=0),
                                                       torch.stack([n.n_invalid for n in self.nb], dim=0), _stack_scores([n.pooled for n in self.nb]))
        return res


@torch.no_grad()
def score_rollout(model, x0: torch.Tensor, truth, n_steps: int, coszen: torch.Tensor | None = None, n_invar: int = 0,
                  scorer: ForecastScorer | None = None, keep_forecast: bool = False, extremes: bool = False,
                  spectrum: bool = False, events: EventSpec | None = None, neighbourhoods=None, coherence: bool = False) -> RolloutScores:
    """`rollout` with every step's prediction scored against truth[:, s] as soon as it is written.  truth: [B, n_steps, Cout, H, W]
    (normalised as the model's output) or a callable s -> [B, Cout, H, W].  scorer: a ForecastScorer (default: no climatology, so
    no ACC; normalised units).  Unless keep_forecast, the predictions live in a two-slot ring [B, 2 Cout, H, W]: memory does not grow
    with n_steps.  -> RolloutScores(rmse [n_steps, Cout] and acc [n_steps, Cout] | None: batch means (rmse x the scorer's stds);
    rmse_samples, acc_samples [n_steps, B, Cout]; forecast [B, n_steps, Cout, H, W] | None;
    tqe [n_steps, B, Cout] | None).  extremes: every step's prediction also goes through scorer.quantile_error against that step's truth
    (the top-quantile error, tqe).  spectrum: every step's prediction and truth also go through scorer.power_spectrum ->
    spectrum = RolloutSpectrum(pred, truth [n_steps, Cout, lmax = H]: batch-mean degree power in the scorer's normalised units; ratio
    [n_steps, B, Cout]: small_scale_power_ratio per sample), else None.  The predictions are `rollout`'s, bit for bit.
    scorer may be a RegriddedScorer: truth stays on the model's grid and both are regridded before every score (no spectrum then).
    events: an EventSpec(kind "anomaly" | "quantile", levels, below): every step also goes through scorer.event_score with the thresholds
    scorer.event_thresholds names (offsets from the climatology, or that step's spatial quantiles of the analysis) -> the attribute
    `events`, a RolloutEvents; every other result is what the call without it returns, bit for bit.
    neighbourhoods: with events, half-widths (r, ...) in grid points: every step also goes through scorer.neighbourhood_score with the
    same thresholds (the fractions skill score per scale) -> the attribute `neighbourhoods`, a RolloutNeighbourhoods.
    coherence: every step's prediction and truth also go through scorer.spectral_coherence -> the attribute `coherence`, a
    RolloutCoherence(coherence [n_steps, Cout, lmax = H] fp64: the batch mean of C / sqrt(P_pred P_truth) per degree; scale [n_steps, B, Cout]:
    utils/sht.py::coherence_scale per sample, the degree down to which the forecast is in the right place; level), else None."""
    net = model.model if hasattr(model, "model") else model
    B, _, H, W = x0.shape
    Cout = net.out_chans
    if scorer is None:
        scorer = ForecastScorer(H, W, Cout, x0.device)
    _check_events("score_rollout", events, scorer, neighbourhoods)
    if coherence and isinstance(scorer, RegriddedScorer):
        raise ValueError("score_rollout: coherence=True needs a ForecastScorer (degree spectra are taken on the model's own grid)")
    if spectrum and isinstance(scorer, RegriddedScorer):
        raise ValueError("score_rollout: spectrum=True needs a ForecastScorer (degree spectra are taken on the model's own grid)")
    out, coff_of, forecast = _ring(B, n_steps, Cout, H, W, x0.device, keep_forecast)
    steps = _StepScores(scorer, n_steps, B, Cout, H, x0.device, events, extremes, spectrum, neighbourhoods, coherence)
    for s in _rollout_steps(net, x0, n_steps, coszen, n_invar, out, coff_of):
        tar = _truth_at(truth, s, x0.device)
        steps.add(s, scorer, out, tar, coff_of(s))
        steps.add_events(s, scorer, out, tar, coff_of(s))
    return steps.result(forecast)


def perturb_initial_condition(x0: torch.Tensor, n_members: int, amplitude: float, seed: int, n_fields: int, kind: str = "white",
                              length_scale_km: float | None = None) -> torch.Tensor:
    """x0 [B, Cin, H, W] (fields | zenith | invariants) -> the M = n_members initial conditions [M B, Cin, H, W], member-major (row m B + b).
    Member 0 is x0 bit for bit (the control); the members 1 .. M - 1 add
        amplitude * torch.randn((M - 1) B, n_fields, H, W, generator=torch.Generator(x0.device).manual_seed(seed))
    to the first n_fields channels.  The other channels (cos-zenith, invariants) are x0's bit for bit in every member.
    kind="spherical": isotropic noise on the sphere with a Gaussian correlation of length_scale_km, zero global mean and unit variance at
    every point (utils/sht.py::gaussian_noise_spectrum, spherical_noise) in place of the white noise.  The rows r = (member - 1) B + b
    are drawn one at a time in ascending order from the same single generator,
        z = torch.randn(W // 2 + 1, 2 n_fields, H, generator=gen)          fp32, the coefficient layout [mmax, 2 planes, lmax]
    and amplitude * spherical_noise(z, sigma, W) is added to the row's field channels."""
    M = int(n_members)
    B, Cin, H, W = x0.shape
    if M < 1 or not 0 <= n_fields <= Cin:
        raise ValueError(f"perturb_initial_condition: {M} members, {n_fields} fields of {Cin} channels")
    if kind not in ("white", "spherical") or (kind == "spherical") != (length_scale_km is not None):
        raise ValueError(f"perturb_initial_condition: kind {kind!r} with length_scale_km {length_scale_km} (\"white\" takes none, \"spherical\" needs one)")
    out = x0.repeat(M, 1, 1, 1)
    if M > 1 and n_fields:
        gen = torch.Generator(device=x0.device).manual_seed(int(seed))
        if kind == "white":
            noise = torch.randn((M - 1) * B, n_fields, H, W, generator=gen, device=x0.device, dtype=x0.dtype)
            out[B:, :n_fields] += amplitude * noise
        else:
            from .utils import sht
            sigma = sht.gaussian_noise_spectrum(H, W, length_scale_km)
            for r in range((M - 1) * B):
                z = torch.randn(W // 2 + 1, 2 * n_fields, H, generator=gen, device=x0.device, dtype=torch.float32)
                out[B + r, :n_fields] += (amplitude * sht.spherical_noise(z, sigma, W)).to(x0.dtype)
    return out


class EnsembleRolloutScores(namedtuple("EnsembleRolloutScores", "crps fair_crps spread ens_rmse crps_samples fair_crps_samples spread_samples "
                                       "ens_rmse_samples hist forecast control", defaults=(None,))):
    """ensemble_rollout's answer.  The tuple keeps its eleven fields; `events` rides along as an attribute: None, or the
    EnsembleRolloutEvents of ensemble_rollout(..., events=spec); so does `neighbourhoods`: None, or the EnsembleRolloutNeighbourhoods of
    ensemble_rollout(..., events=spec, ensemble_neighbourhoods=scales)."""
    events = None
    neighbourhoods = None


@torch.no_grad()
def ensemble_rollout(model, x0: torch.Tensor, truth, n_steps: int, n_members: int, amplitude: float, seed: int = 0,
                     coszen: torch.Tensor | None = None, n_invar: int = 0, scorer: ForecastScorer | None = None,
                     member_batch: int | None = None, keep_forecast: bool = False, n_fields: int | None = None,
                     score_control: bool = False, perturbation_kind: str = "white",
                     length_scale_km: float | None = None, events: EventSpec | None = None, neighbourhoods=None,
                     ensemble_neighbourhoods=None, member_neighbourhoods: bool = False) -> EnsembleRolloutScores:
    """`score_rollout` for an ensemble: x0 [B, Cin, H, W] is perturbed into M = n_members initial conditions (perturb_initial_condition,
    which perturbation_kind and length_scale_km are handed to; n_fields defaults to Cin - n_invar - (1 if coszen is given)), all members are rolled out and every step is scored against truth[:, s]
    by scorer.ensemble_score as soon as all members have written it.  truth, scorer: as in score_rollout; coszen [B, n_steps - 1, H, W] is
    repeated for every member.  Unless keep_forecast the predictions live in a two-slot ring [M B, 2 Cout, H, W], scored where they lie.
    member_batch: members per model call (default: all M at once); the chunks advance in lockstep, one step at a time.  With one chunk
    the forecasts are rollout(model, perturb_initial_condition(...), n_steps, coszen.repeat(M, 1, 1, 1), n_invar)'s bit for bit.
    -> EnsembleRolloutScores(crps, fair_crps, spread, ens_rmse [n_steps, Cout]: batch means (the scorer's stds on crps, spread, ens_rmse);
    their _samples [n_steps, B, Cout]; hist [n_steps, B, Cout, M + 1] int32; forecast [M B, n_steps, Cout, H, W] | None;
    control: with score_control, the RolloutScores of member 0 -- the deterministic forecast -- from scorer.score, else None).
    events: an EventSpec, as in score_rollout: every step also goes through scorer.ensemble_event_score (Brier score, reliability, ROC area
    of the exceedance probabilities) -> the attribute `events`, an EnsembleRolloutEvents; with score_control the control carries its own
    RolloutEvents (the contingency tables of member 0).  Every other result is what the call without it returns, bit for bit.
    ensemble_neighbourhoods: with events, half-widths (r, ...) in grid points: every step also goes through
    scorer.ensemble_neighbourhood_score with the same thresholds, reading the ring slot in place (the probabilistic fractions skill score
    per scale) -> the attribute `neighbourhoods`, an EnsembleRolloutNeighbourhoods; member_neighbourhoods adds the member and dispersion
    rows (eFSS / dFSS).  Every other result stays bit for bit.
    neighbourhoods: refused.  That keyword names the fractions skill score of ONE forecast (score_rollout); the ensemble's is
    ensemble_neighbourhoods=."""
    if neighbourhoods is not None:
        raise ValueError("ensemble_rollout: neighbourhoods= names the fractions skill score of one forecast (score_rollout(..., events=, "
                         "neighbourhoods=)); the ensemble (probabilistic) score is ensemble_neighbourhoods=")
    if member_neighbourhoods and ensemble_neighbourhoods is None:
        raise ValueError("ensemble_rollout: member_neighbourhoods adds to ensemble_neighbourhoods=: give the scales")
    net = model.model if hasattr(model, "model") else model
    B, Cin, H, W = x0.shape
    M, Cout = int(n_members), net.out_chans
    if M < 2:
        raise ValueError(f"ensemble_rollout: {M} members (an ensemble has at least 2)")
    K = M if member_batch is None else int(member_batch)
    if K < 1:
        raise ValueError(f"ensemble_rollout: member_batch {member_batch}")
    if scorer is None:
        scorer = ForecastScorer(H, W, Cout, x0.device)
    _check_events("ensemble_rollout", events, scorer, ensemble_neighbourhoods)
    nb_scales, nb = (None if ensemble_neighbourhoods is None else tuple(ensemble_neighbourhoods)), []
    if n_fields is None:
        n_fields = Cin - n_invar - int(coszen is not None)
    xe = perturb_initial_condition(x0, M, amplitude, seed, n_fields, perturbation_kind, length_scale_km)
    out, coff_of, forecast = _ring(M * B, n_steps, Cout, H, W, x0.device, keep_forecast)
    chunks = []
    for m0 in range(0, M, K):
        r0, r1 = m0 * B, min(m0 + K, M) * B
        cz = None if coszen is None else coszen.repeat((r1 - r0) // B, 1, 1, 1)
        chunks.append(_rollout_steps(net, xe[r0:r1], n_steps, cz, n_invar, out[r0:r1], coff_of))
    mean = {k: torch.empty(n_steps, Cout, dtype=torch.float32, device=x0.device) for k in ("crps", "fair_crps", "spread", "ens_rmse")}
    samp = {k: torch.empty(n_steps, B, Cout, dtype=torch.float32, device=x0.device) for k in mean}
    hist, ev = torch.empty(n_steps, B, Cout, M + 1, dtype=torch.int32, device=x0.device), []
    ctl = _StepScores(scorer, n_steps, B, Cout, H, x0.device, events) if score_control else None      # member 0: the deterministic forecast
    for s in range(n_steps):
        for ch in chunks:
            next(ch)
        tar = _truth_at(truth, s, x0.device)
        r = scorer.ensemble_score(out, tar, M, coff_ens=coff_of(s))
        for k in mean:
            mean[k][s], samp[k][s] = getattr(r, k + "_mean"), getattr(r, k)
        hist[s] = r.hist
        thr = None if events is None else scorer.event_thresholds(events, tar)
        if events is not None:
            ev.append((thr, scorer.ensemble_event_score(out, tar, M, thr, anomaly=events.kind == "anomaly", below=events.below, coff_ens=coff_of(s))))
        if nb_scales is not None:
            nb.append(scorer.ensemble_neighbourhood_score(out, tar, M, thr, nb_scales, anomaly=events.kind == "anomaly", below=events.below,
                                                          coff_ens=coff_of(s), members=member_neighbourhoods))
        if ctl is not None:
            ctl.add_events(s, scorer, out[:B], tar, coff_of(s), thr)
            ctl.add(s, scorer, out[:B], tar, coff_of(s))
    res = EnsembleRolloutScores(*mean.values(), *samp.values(), hist, forecast, None if ctl is None else ctl.result(None))      # (the fields' order)
    if events is not None:
        stack = lambda i: torch.stack([e[i] for _, e in ev], dim=0)      # noqa: E731
        res.events = EnsembleRolloutEvents(events, [t for t, _ in ev], stack(0), stack(1), stack(2), stack(3),
                                           _stack_scores([{**e.pooled, **e.reliability} for _, e in ev]))
    if nb_scales is not None:
        stack = lambda k: torch.stack([getattr(n, k) for n in nb], dim=0)      # noqa: E731
        more = (stack("member_rows"), stack("dispersion_rows"), _stack_scores([n.member_scores for n in nb]),
                _stack_scores([n.dispersion_scores for n in nb])) if member_neighbourhoods else ()
        res.neighbourhoods = EnsembleRolloutNeighbourhoods(nb_scales, stack("rows"), stack("n_invalid"), _stack_scores([n.pooled for n in nb]), *more)
    return res


def lead_time_table(scores: RolloutScores, names, hours_per_step: float = 6.0, ensemble: EnsembleRolloutScores | None = None) -> str:
    """one line per lead time: RMSE (and ACC, and the batch-mean top-quantile error and small-scale power ratio when scored) of the named channels;
    names: [(column title, channel index)]; lcoh_<name>, the batch-mean coherence scale, follows when the coherence was scored.  ensemble: the crps_, spread_ and ens_rmse_ columns of an ensemble_rollout follow.  Scored
    events add the equitable threat score of every threshold k, ets<k>_<name>, and -- for an ensemble -- its Brier score, bs<k>_<name>;
    scored neighbourhoods add the fractions skill score of every threshold k and scale r, fss<k>_r<r>_<name>, behind them; an ensemble's
    neighbourhoods add pfss<k>_r<r>_<name> and, with member scores, efss... and dfss... columns behind those."""
    rm, ac = scores.rmse.cpu().numpy(), None if scores.acc is None else scores.acc.cpu().numpy()
    tq = None if scores.tqe is None else scores.tqe.mean(dim=1).cpu().numpy()
    sr = None if scores.spectrum is None else scores.spectrum.ratio.mean(dim=1).cpu().numpy()
    lc = None if scores.coherence is None else scores.coherence.scale.double().mean(dim=1).cpu().numpy()
    cols = [f"rmse_{n}" for n, _ in names] + ([f"acc_{n}" for n, _ in names] if ac is not None else []) + \
        ([f"tqe_{n}" for n, _ in names] if tq is not None else []) + ([f"ssr_{n}" for n, _ in names] if sr is not None else []) + \
        ([f"lcoh_{n}" for n, _ in names] if lc is not None else [])
    ens = [] if ensemble is None else [(k, getattr(ensemble, k).cpu().numpy()) for k in ("crps", "spread", "ens_rmse")]
    cols += [f"{k}_{n}" for k, _ in ens for n, _ in names]
    if scores.events is not None:
        ens.append(("ets", scores.events.scores["ets"].cpu().numpy()))
    if ensemble is not None and ensemble.events is not None:
        ens.append(("bs", ensemble.events.scores["brier"].cpu().numpy()))
    evs = [(k, v) for k, v in ens if v.ndim == 3]
    ens = [(k, v) for k, v in ens if v.ndim == 2]
    cols += [f"{k}{j}_{n}" for k, v in evs for j in range(v.shape[2]) for n, _ in names]
    nbh = scores.neighbourhoods
    fss = None if nbh is None else nbh.scores["fss"].cpu().numpy()             # [n_steps, C, K, S]
    if fss is not None:
        cols += [f"fss{j}_r{r}_{n}" for j in range(fss.shape[2]) for r in nbh.scales for n, _ in names]
    nbs = []                                                                   # (scores [n_steps, C, K, S]) of the ensemble's neighbourhoods
    enb = None if ensemble is None else ensemble.neighbourhoods
    if enb is not None:
        nbs = [("pfss", enb.scores["pfss"])] + ([("efss", enb.member_scores["fss"]), ("dfss", enb.dispersion_scores["fss"])]
                                                if enb.member_scores is not None else [])
        nbs = [(k, v.cpu().numpy()) for k, v in nbs]
        cols += [f"{k}{j}_r{r}_{n}" for k, v in nbs for j in range(v.shape[2]) for r in enb.scales for n, _ in names]
    lines = ["lead_h " + " ".join(f"{c:>12s}" for c in cols)]
    for s in range(rm.shape[0]):
        vals = [rm[s, i] for _, i in names] + ([ac[s, i] for _, i in names] if ac is not None else []) + \
            ([tq[s, i] for _, i in names] if tq is not None else []) + ([sr[s, i] for _, i in names] if sr is not None else []) + \
            ([lc[s, i] for _, i in names] if lc is not None else []) + [v[s, i] for _, v in ens for _, i in names] + [v[s, i, j] for _, v in evs for j in range(v.shape[2]) for _, i in names]
        if fss is not None:
            vals += [fss[s, i, j, q] for j in range(fss.shape[2]) for q in range(fss.shape[3]) for _, i in names]
        vals += [v[s, i, j, q] for _, v in nbs for j in range(v.shape[2]) for q in range(v.shape[3]) for _, i in names]
        lines.append(f"{hours_per_step * (s + 1):6.0f} " + " ".join(f"{v:12.5f}" for v in vals))
    return "\n".join(lines)


class _Parser(argparse.ArgumentParser):
    """the flags that only make sense together are checked where the command line is parsed: a wrong combination is a parser error"""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if a.spectrum_out and not a.spectrum:
            self.error("--spectrum-out needs --spectrum")
        if a.coherence and not a.truth:
            self.error("--coherence relates the forecast to the verifying analysis degree by degree: it needs --truth")
        if a.coherence and a.score_grid is not None:
            self.error("--score-grid scores on a coarser grid; --coherence is taken on the model's own grid: run them separately")
        if a.score_grid is not None:
            if not a.truth:
                self.error("--score-grid names the grid the scores are taken on: it needs --truth")
            if a.spectrum:
                self.error("--score-grid scores on a coarser grid; --spectrum is taken on the model's own grid: run them separately")
            try:
                grid_for_degrees(a.score_grid)
            except ValueError as e:
                self.error(f"--score-grid: {e}")
        if a.event_anomaly is not None and a.event_quantile is not None:
            self.error("--event-anomaly and --event-quantile name the thresholds in two ways: give one of them")
        if a.event_below and a.event_anomaly is None and a.event_quantile is None:
            self.error("--event-below turns the event of --event-anomaly / --event-quantile round: it needs one of them")
        if (a.event_anomaly is not None or a.event_quantile is not None) and not a.truth:
            self.error("--event-anomaly / --event-quantile score events against the verifying analysis: they need --truth")
        if a.event_quantile is not None and not all(0.0 <= q <= 1.0 for q in a.event_quantile):
            self.error("--event-quantile: levels within 0 .. 1")
        if a.event_scales is not None:
            if a.event_anomaly is None and a.event_quantile is None:
                self.error("--event-scales takes neighbourhoods around the events of --event-anomaly / --event-quantile: it needs one of them")
            if a.ensemble is not None:
                self.error("--event-scales (the fractions skill score) is scored for a single forecast: run it without --ensemble, or give "
                           "--ensemble-scales for the ensemble's probabilistic score")
            r = a.event_scales
            if any(y <= x for x, y in zip(r, r[1:])) or r[0] < 0 or r[-1] > 32:
                self.error("--event-scales: strictly ascending half-widths in grid points, within 0 .. 32")
        if a.ensemble_scales is not None:
            if a.event_anomaly is None and a.event_quantile is None:
                self.error("--ensemble-scales takes neighbourhoods around the events of --event-anomaly / --event-quantile: it needs one of them")
            r = a.ensemble_scales
            if any(y <= x for x, y in zip(r, r[1:])) or r[0] < 0 or r[-1] > 32:
                self.error("--ensemble-scales: strictly ascending half-widths in grid points, within 0 .. 32")
        if a.ensemble_member_scores and a.ensemble_scales is None:
            self.error("--ensemble-member-scores adds to --ensemble-scales: it needs it")
        if a.ensemble is None:
            for flag, v in (("--perturbation", a.perturbation), ("--seed", a.seed), ("--member-batch", a.member_batch),
                            ("--perturbation-scale", a.perturbation_scale), ("--ensemble-scales", a.ensemble_scales)):
                if v is not None:
                    self.error(f"{flag} needs --ensemble")
            return a
        if not a.truth:
            self.error("--ensemble scores the members against the verifying analysis: it needs --truth")
        if a.out:
            self.error("--ensemble keeps no forecast: it cannot be combined with --out")
        if a.extremes:
            self.error("--extremes is scored for a single forecast: run it without --ensemble")
        if a.spectrum:
            self.error("--spectrum is scored for a single forecast: run it without --ensemble")
        if a.coherence:
            self.error("--coherence is scored for a single forecast: run it without --ensemble")
        if not 2 <= a.ensemble <= 64:
            self.error("--ensemble: 2 .. 64 members")
        if a.perturbation is None:
            self.error("--ensemble needs --perturbation (the amplitude of the initial-condition noise, in normalised units)")
        if a.member_batch is not None and a.member_batch < 1:
            self.error("--member-batch: at least one member per model call")
        if a.perturbation_scale is not None and not a.perturbation_scale > 0:
            self.error("--perturbation-scale: a correlation length in km, above 0")
        return a


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(description=__doc__.split("\n")[0])
    ap.add_argument("--registry", required=True, help="model folder with hyperparams.yaml + weights.tar")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--init", default=None, help=".npy [B, Cin, H, W] normalised initial condition (default: seeded N(0,1))")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trust-checkpoint", action="store_true", help="read weights.tar with the full unpickler (runs code from the file)")
    ap.add_argument("--truth", default=None, help=".npy [B, steps, Cout, H, W] normalised verifying analysis: score every lead time against it")
    ap.add_argument("--climatology", default=None, help=".npy time means [1, Call, Hfull, Wfull] for ACC (default: the registry's time_means.npy, "
                                                        "else the hyper-parameters' time_means_path)")
    ap.add_argument("--scores-out", default=None, help="write the lead-time scores as JSON")
    ap.add_argument("--extremes", action="store_true", help="with --truth: also score the top-quantile error (tqe_<name> columns, \"tqe\" key)")
    ap.add_argument("--spectrum", action="store_true", help="with --truth: also the spherical-harmonic degree power of forecast and analysis; "
                                                            "ssr_<name> columns (small-scale power ratio), \"ssr\" key")
    ap.add_argument("--coherence", action="store_true", help="with --truth: also the spectral coherence of forecast and analysis per degree and "
                                                             "the degree down to which it stays at or above 0.5; lcoh_<name> columns, "
                                                             "\"coherence\" key; with --spectrum-out a coherence array [steps, Cout, lmax]")
    ap.add_argument("--spectrum-out", default=None, metavar="FILE.npz", help="with --spectrum: write the arrays degree [lmax], pred and truth "
                                                                             "[steps, Cout, lmax] (batch-mean degree power)")
    ap.add_argument("--score-grid", type=float, default=None, metavar="DEG", help="with --truth: regrid forecast and analysis (first-order "
                                                                                  "conservative) to the DEG-degree global grid and score there "
                                                                                  "with cell-area weights (1.5: 121 x 240, the WeatherBench 2 "
                                                                                  "scorecards' grid; 5.625: 32 x 64); the truth file stays on the "
                                                                                  "model's grid")
    ap.add_argument("--event-anomaly", type=float, nargs="+", default=None, metavar="S", help="with --truth and a climatology: score the events "
                    "\"more than S above the climatology\" (normalised units; one or more thresholds): ets<k>_<name> columns, with --ensemble "
                    "also bs<k>_<name> (Brier score), \"events\" key")
    ap.add_argument("--event-quantile", type=float, nargs="+", default=None, metavar="Q", help="with --truth: score the events \"above the Q "
                    "quantile of the verifying analysis\" (its own spatial quantile per lead time, sample and channel); not with --event-anomaly")
    ap.add_argument("--event-below", action="store_true", help="with --event-anomaly / --event-quantile: the event is \"below\" the threshold")
    ap.add_argument("--event-scales", type=int, nargs="+", default=None, metavar="R", help="with --event-anomaly / --event-quantile: also the "
                    "fractions skill score of those events over boxes of 2 R + 1 grid points (ascending half-widths within 0 .. 32, on the "
                    "--score-grid if given): fss<k>_r<R>_<name> columns, \"fss\" key")
    ap.add_argument("--ensemble-scales", type=int, nargs="+", default=None, metavar="R", help="with --ensemble and --event-anomaly / "
                    "--event-quantile: the probabilistic fractions skill score of the members' neighbourhood probabilities over boxes of 2 R + 1 "
                    "grid points (ascending half-widths within 0 .. 32): pfss<k>_r<R>_<name> columns, \"pfss\" key")
    ap.add_argument("--ensemble-member-scores", action="store_true", help="with --ensemble-scales: also the mean member's FSS against the "
                    "analysis and against the control (efss / dfss columns and keys: spatial skill and spread)")
    ap.add_argument("--ensemble", type=int, default=None, metavar="M", help="with --truth: roll out M members from perturbed initial conditions "
                                                                            "(member 0 is the control) and score CRPS, spread and ensemble-mean RMSE "
                                                                            "(crps_/spread_/ens_rmse_<name> columns, \"ensemble\" key)")
    ap.add_argument("--perturbation", type=float, default=None, metavar="A", help="with --ensemble: amplitude of the N(0, 1) noise added to the fields")
    ap.add_argument("--seed", type=int, default=None, help="with --ensemble: seed of the noise (default 0)")
    ap.add_argument("--member-batch", type=int, default=None, metavar="K", help="with --ensemble: members per model call (default: all at once)")
    ap.add_argument("--perturbation-scale", type=float, default=None, metavar="KM", help="with --ensemble: the noise is isotropic on the sphere with a "
                                                                                        "Gaussian correlation of this length (default: white per grid point)")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    dev = torch.device("cuda:0")
    model, p, stats = load_registry_model(a.registry, dev, trust_checkpoint=a.trust_checkpoint)
    H, W = p["img_size"]
    n_invar = 2 * int(bool(p["add_landmask"])) + int(bool(p["add_orography"]))
    if a.init:
        x0 = torch.from_numpy(np.load(a.init)).float().to(dev)
    else:
        x0 = torch.randn(1, p["n_in_channels"], H, W, generator=torch.Generator().manual_seed(0)).to(dev)
    cz = None
    if p["add_zenith"]:
        from .utils.data_loader_era5 import cos_zenith
        cz = torch.stack([cos_zenith(2018, 6.0 * (s + 1), H, W) for s in range(a.steps - 1)], 0).unsqueeze(0).expand(x0.shape[0], -1, -1, -1).to(dev) \
            if a.steps > 1 else None
    if a.truth:
        return _score_main(a, model, p, stats, x0, cz, n_invar)
    y = rollout(model, x0, a.steps, cz, n_invar)
    print(f"forecast {tuple(y.shape)}: per-step rms " + " ".join(f"{float(y[:, s].square().mean().sqrt()):.4f}" for s in range(a.steps)))
    if a.out:
        np.save(a.out, y.cpu().numpy())


def _score_main(a, model, p, stats, x0, cz, n_invar):
    """--truth: roll out, score every lead time, print the table of the tracked channels (default u10m, v10m as the Trainer)"""
    H, W = p["img_size"]
    chans = np.asarray(p["out_channels"])
    reg_tm = os.path.join(a.registry, "time_means.npy")
    pc = _Params(p)
    pc["time_means_path"] = a.climatology or (reg_tm if os.path.isfile(reg_tm) else p.get("time_means_path"))
    means, stds = stats if stats is not None else (None, None)
    clim = load_climatology(pc, means=means, stds=stds)
    phys = None if stds is None else stds[0, chans, 0, 0]
    grid = None
    if a.score_grid is not None:
        grid = grid_for_degrees(a.score_grid)
        scorer = RegriddedScorer(Regridder(model_grid(H, W), grid, x0.device), len(chans), climatology=clim, stds=phys)
    else:
        scorer = ForecastScorer(H, W, len(chans), x0.device, climatology=clim, stds=phys)
    truth = np.load(a.truth, mmap_mode="r")              # read step by step: the whole array need not fit in host memory
    if truth.ndim != 5 or truth.shape[1] < a.steps:
        raise ValueError(f"--truth: expected [B, >= {a.steps}, Cout, H, W], got {truth.shape}")
    truth_of = lambda s: torch.from_numpy(np.array(truth[:, s], dtype=np.float32)).to(x0.device)      # noqa: E731
    spec = None
    if a.event_anomaly is not None:
        if clim is None:
            raise ValueError("--event-anomaly: thresholds relative to the climatology need one (--climatology, or time_means.npy in the registry)")
        spec = EventSpec("anomaly", tuple(a.event_anomaly), a.event_below)
    elif a.event_quantile is not None:
        spec = EventSpec("quantile", tuple(a.event_quantile), a.event_below)
    ens = None
    if a.ensemble is not None:
        # one rollout of all members: member 0 is the unperturbed forecast, scored as score_rollout scores it
        ens = ensemble_rollout(model, x0, truth_of, a.steps, a.ensemble, a.perturbation, a.seed or 0, cz, n_invar, scorer,
                               member_batch=a.member_batch, n_fields=len(p["in_channels"]), score_control=True,
                               perturbation_kind="white" if a.perturbation_scale is None else "spherical", length_scale_km=a.perturbation_scale,
                               events=spec, ensemble_neighbourhoods=None if a.ensemble_scales is None else tuple(a.ensemble_scales),
                               member_neighbourhoods=a.ensemble_member_scores)
        sc = ens.control
    else:
        sc = score_rollout(model, x0, truth_of, a.steps, cz, n_invar, scorer, keep_forecast=bool(a.out), extremes=a.extremes, spectrum=a.spectrum,
                           events=spec, neighbourhoods=None if a.event_scales is None else tuple(a.event_scales), coherence=a.coherence)
    if "track_channels" in p and "channel_names" in p:
        names = [(v, list(p["channel_names"]).index(v)) for v in p["track_channels"]]
    else:
        names = [(v, i) for i, v in enumerate(("u10m", "v10m")) if i < len(chans)]
    print(f"scores in {'physical' if stds is not None else 'normalised'} units, {'with' if clim is not None else 'no climatology: without'} ACC")
    if grid is not None:
        print(f"scored on the {a.score_grid:g} degree grid ({grid.nlat} x {grid.nlon}, {'both poles' if grid.poles else 'no pole rows'}) after "
              "first-order conservative regridding, cell-area weights")
    print(lead_time_table(sc, names, ensemble=ens))
    if a.scores_out:
        doc = {"lead_hours": [6.0 * (s + 1) for s in range(a.steps)], "rmse": sc.rmse.cpu().tolist(),
               "acc": None if sc.acc is None else sc.acc.cpu().tolist(), "tracked": dict(names)}
        if grid is not None:
            doc["grid"] = {"degrees": a.score_grid, "nlat": grid.nlat, "nlon": grid.nlon, "poles": grid.poles, "weights": "cell-area"}
        if sc.tqe is not None:
            doc["tqe"] = sc.tqe.mean(dim=1).cpu().tolist()
        if sc.spectrum is not None:
            doc["ssr"] = sc.spectrum.ratio.mean(dim=1).cpu().tolist()
        if sc.coherence is not None:
            # per lead time and channel: the batch mean of the degree down to which forecast and analysis cohere at `level` or better
            doc["coherence"] = {"lcoh": sc.coherence.scale.double().mean(dim=1).cpu().tolist(), "level": sc.coherence.level}
        if ens is not None:
            doc["ensemble"] = {"members": a.ensemble, "crps": ens.crps.cpu().tolist(), "fair_crps": ens.fair_crps.cpu().tolist(),
                               "spread": ens.spread.cpu().tolist(), "ens_rmse": ens.ens_rmse.cpu().tolist(),
                               "spread_skill": spread_skill_ratio(ens.spread, ens.ens_rmse, a.ensemble).cpu().tolist()}
        if sc.events is not None:
            # pooled over the batch per lead time: the table [steps, C, K, 4] and its scores [steps, C, K]
            doc["events"] = {"kind": spec.kind, "levels": list(spec.levels), "below": bool(spec.below),
                             "table": sc.events.table.to(torch.float64).sum(dim=1).cpu().tolist(),
                             **{k: v.cpu().tolist() for k, v in sc.events.scores.items()}}
            if ens is not None:
                doc["events"].update({k: ens.events.scores[k].cpu().tolist()
                                      for k in ("brier", "fair_brier", "brier_skill", "reliability", "resolution", "roc_area")})
        if sc.neighbourhoods is not None:
            # pooled over the batch per lead time: fss [steps, C, K, S], fss_uniform and useful_scale (a half-width, or -1) [steps, C, K]
            doc["fss"] = {"scales": list(sc.neighbourhoods.scales),
                          **{k: sc.neighbourhoods.scores[k].cpu().tolist() for k in ("fss", "fss_uniform", "useful_scale")}}
        if ens is not None and ens.neighbourhoods is not None:
            # pooled over the batch per lead time: pfss [steps, C, K, S]; efss / dfss likewise with --ensemble-member-scores
            nb = ens.neighbourhoods
            doc["pfss"] = {"scales": list(nb.scales), **{k: nb.scores[k].cpu().tolist() for k in ("pfss", "fss_uniform", "useful_scale")}}
            if nb.member_scores is not None:
                doc["pfss"].update(efss=nb.member_scores["fss"].cpu().tolist(), dfss=nb.dispersion_scores["fss"].cpu().tolist())
        with open(a.scores_out, "w") as f:
            json.dump(doc, f)
    if a.spectrum_out:
        more = {} if sc.coherence is None else {"coherence": sc.coherence.coherence.cpu().numpy()}
        np.savez(a.spectrum_out, degree=np.arange(H), pred=sc.spectrum.pred.cpu().numpy(), truth=sc.spectrum.truth.cpu().numpy(), **more)
    if a.out:
        np.save(a.out, sc.forecast.cpu().numpy())


if __name__ == "__main__":
    main()
