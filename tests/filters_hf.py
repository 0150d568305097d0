"""HF's sampled warper chain in fp64, for the tests of generate(filters=...): the installed transformers classes, in the order
GenerationMixin._get_logits_processor builds them."""
import numpy as np
import torch
from transformers.generation import logits_process as LP

# (temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff): the eight families of the kernel test ...
FAMILIES = [(1.0, 0, 1.0, 0.05, 1.0, 0.0, 0.0),
            (0.7, 50, 0.9, 0.1, 1.0, 0.0, 0.0),
            (1.0, 0, 1.0, None, 0.9, 0.0, 0.0),
            (0.8, 50, 1.0, None, 0.5, 0.0, 0.0),
            (1.0, 0, 1.0, None, 1.0, 3e-4, 0.0),
            (1.0, 0, 1.0, None, 1.0, 0.0, 2e-3),
            (0.9, 0, 0.95, 0.02, 0.95, 1e-4, 1e-3),
            (0.2, 50, 1.0, 0.05, 0.9, 0.0, 0.0)]
# ... and three harsh ones for the rules alone
HARSH = [(1.0, 0, 1.0, None, 0.3, 1e-2, 0.0),
         (1.0, 0, 1.0, 0.3, 0.2, 0.0, 5e-2),
         (0.2, 50, 0.9, 0.5, 0.9, 0.1, 0.1)]


def filters_of(family):
    from video_llava_amd.sample_filters import SampleFilters
    _, _, _, min_p, typical, eps, eta = family
    return SampleFilters(min_p=min_p, typical_p=typical, epsilon_cutoff=eps, eta_cutoff=eta)


def hf_front(scores, temperature, top_k, top_p):
    """scores [B, V] (fp64 tensor; repetition penalty already applied) after HF's temperature / top-k / top-p warpers."""
    y = scores.double()
    ids = torch.zeros(y.shape[0], 1, dtype=torch.long)
    if temperature != 1.0:
        y = LP.TemperatureLogitsWarper(float(temperature))(ids, y)
    if top_k and top_k > 0:
        y = LP.TopKLogitsWarper(int(top_k))(ids, y)
    if top_p < 1.0:
        y = LP.TopPLogitsWarper(float(top_p))(ids, y)
    return y


def hf_tail(y, filters):
    """y [B, V] fp64 after hf_front -> HF's min_p / typical / epsilon / eta warpers, each built exactly when generate() builds it."""
    ids = torch.zeros(y.shape[0], 1, dtype=torch.long)
    if filters.min_p is not None:
        y = LP.MinPLogitsWarper(float(filters.min_p))(ids, y)
    if filters.typical_p is not None and filters.typical_p < 1.0:
        y = LP.TypicalLogitsWarper(float(filters.typical_p))(ids, y)
    if filters.epsilon_cutoff is not None and 0.0 < filters.epsilon_cutoff < 1.0:
        y = LP.EpsilonLogitsWarper(float(filters.epsilon_cutoff))(ids, y)
    if filters.eta_cutoff is not None and 0.0 < filters.eta_cutoff < 1.0:
        w = LP.EtaLogitsWarper(float(filters.eta_cutoff))
        w.epsilon = w.epsilon.double()          # the class keeps its threshold in fp32
        y = w(ids, y)
    return y


def hf_kept(scores, family):
    """Kept masks [B, V] (numpy bool) of HF's whole sampled chain on fp64 scores."""
    t, k, p = family[:3]
    return torch.isfinite(hf_tail(hf_front(scores, t, k, p), filters_of(family))).numpy()


def chain_kept(scores, family, **perturb):
    """The same from this package's rules: HF's front, then sample_filters.filter_chain row by row."""
    from video_llava_amd.sample_filters import filter_chain
    t, k, p = family[:3]
    y = hf_front(scores, t, k, p).numpy()
    f = filters_of(family)
    return np.stack([filter_chain(row, f, **perturb) for row in y])
