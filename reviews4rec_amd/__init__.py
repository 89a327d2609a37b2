"""reviews4rec_amd -- MI355X-native rating-prediction training path for the
review-aware recommenders of noveens/reviews4rec.

Layout
  csrc/            hand-written HIP kernels for gfx950 + the C ABI (include/r4r.h)
  _lib.py          ctypes binding, signatures parsed from the header
  ops.py           torch.autograd glue over the C ABI
  optim.py         fused dense Adam with torch.optim.Adam's surface
  pytorch_models/  drop-in Model(hyper_params) classes (same names as the reference)
  main.py eval.py loss.py data_fast.py hyper_params.py utils.py   host-surface counterparts
  dist.py          one-process-per-GPU data parallelism over RCCL
  recommend.py     catalogue top-K lists and full-catalogue ranks (Catalogue, catalogue_limits, fold_fm,
                   ranking_metrics) over csrc/topk.hip; the same for the ReLU-sum heads of deepconn++ and NeuMF
                   (ReluCatalogue, relu_catalogue_limits, fold_relu_head) over csrc/topk_relu.hip, and for NARRE's
                   product-MLP head (NarreCatalogue, narre_catalogue_limits) over csrc/topk_hmlp.hip, and for the TransNets'
                   ReLU-FM head (TransNetCatalogue, transnet_catalogue_limits, fold_transnet_head) over csrc/topk_rfm.hip,
                   and for MF's product-FM head (MFCatalogue, mf_catalogue_limits, fold_mf_head) over csrc/topk_pfm.hip;
                   slates -- the K best of, and the place of an item among, a candidate list per user, for every class
                   (Catalogue.recommend_among / rank_among, slates_csr, sample_negatives; eval.eval_sampled: the
                   sampled-negative protocol at any number of negatives and any K) over csrc/slate_device.h
"""
__version__ = '0.1.0'


def get_model_class(model_type):
    """Counterpart of the class selection at main.py:349-352."""
    if model_type in ('deepconn', 'deepconn++'):
        from .pytorch_models.DeepCoNN import DeepCoNN as Model
    elif model_type in ('transnet', 'transnet++'):
        from .pytorch_models.TransNet import TransNet as Model
    elif model_type == 'NARRE':
        from .pytorch_models.NARRE import NARRE as Model
    elif model_type in ('bias_only', 'MF', 'MF_dot'):
        from .pytorch_models.MF import MF as Model
    elif model_type == 'NeuMF':                      # GMF / MLP / NeuMF by hyper_params['neumf_stage']
        from .pytorch_models.NeuMF import build as Model
    else:
        raise ValueError('model_type %r is not on the accelerated path' % (model_type,))
    return Model


from .recommend import Catalogue, catalogue_limits, fold_fm, ranking_metrics  # noqa: E402,F401
from .recommend import ReluCatalogue, fold_relu_head, relu_catalogue_limits  # noqa: E402,F401
from .recommend import Explanation, NarreCatalogue, narre_catalogue_limits  # noqa: E402,F401
from .recommend import Phrases, check_explain_words_request, phrase_limits, write_phrases  # noqa: E402,F401
from .recommend import TransNetCatalogue, fold_transnet_head, transnet_catalogue_limits  # noqa: E402,F401
from .recommend import MFCatalogue, fold_mf_head, mf_catalogue_limits  # noqa: E402,F401
from .recommend import sample_negatives, slates_csr  # noqa: E402,F401
from .recommend import PairPhrases, check_explain_pairs_request, write_pair_phrases  # noqa: E402,F401
from .recommend import PairReviews  # noqa: E402,F401
from .recommend import DeletionCurve, LeaveOneOut, WhatIf  # noqa: E402,F401
from .recommend import Counterfactual  # noqa: E402,F401
from .recommend import Shapley  # noqa: E402,F401
from .recommend import DocDeletionCurve, DocLeaveOneOut, check_explain_reviews_request, write_pair_reviews  # noqa: E402,F401
from .eval import eval_catalogue, eval_sampled  # noqa: E402,F401
