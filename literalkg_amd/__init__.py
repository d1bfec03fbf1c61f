"""literalkg_amd -- MI355X (gfx950) native hot path of LiteralKG.

Host code is Python on PyTorch-ROCm and mirrors the reference's nn.Module
surface (``LiteralKG(args, n_entities, n_relations, A_in, num_lit, txt_lit)``,
``model(*input, device=, mode=)``, same ``state_dict`` keys); all arithmetic on
the path runs in hand-written HIP kernels behind the C ABI of
``include/literalkg_hip.h`` (``literalkg_amd/lib/liblkg_hip.so``).  There is no
CPU fallback: importing works anywhere, computing needs the library and a GPU.
"""
from .gate import Gate, GateMul          # noqa: F401
from .model import Aggregator, LiteralKG  # noqa: F401
from .graph import KGStructure           # noqa: F401
from .ranking import KnownTriples, RankResult, evaluate_ranking   # noqa: F401
from .topk import TopKResult, predict_topk   # noqa: F401
from .accepted import AcceptedResult, count_accepted, predict_accepted   # noqa: F401
from .retrieval import AnswerRanks, evaluate_retrieval, rank_answers   # noqa: F401
from .pairmlp import (FoldedMLPHead, count_accepted_mlp, evaluate_mlp_classification, evaluate_mlp_ranking,   # noqa: F401
                      fold_mlp_head, mlp_scores, predict_accepted_mlp, rank_pairs_mlp, score_pairs_mlp)
from .triples import (TripleThresholds, evaluate_triple_classification, fit_triple_thresholds,   # noqa: F401
                      score_triples)
from .relations import (RelationTopK, evaluate_relation_prediction, predict_relations, rank_relations,   # noqa: F401
                        score_relations)
from .one_vs_all import one_vs_all_loss   # noqa: F401
from .kvs_all import distinct_queries, kvs_all_loss, sigmoid_all_loss   # noqa: F401
from .self_adversarial import group_sampled_batch, sampled_sigmoid_loss, self_adversarial_loss   # noqa: F401
from .negatives import (NegativeBatch, NegativeSampler, RelationCardinalities, TripleEpoch, answer_counts,   # noqa: F401
                        relation_cardinalities, sampled_negative_loss, subsampling_weights)
from .relation_loss import relation_loss, relation_softmax_loss   # noqa: F401  (the name relation_loss is the FUNCTION here)
from .gemm_ordered import (current_route, gemm_ordered, gemm_ordered_splits, matmul_ordered,   # noqa: F401  (gemm_ordered: the
                           product_route)                                                      # FUNCTION here, as above)
from .pruned import sample_neighbors   # noqa: F401
from .lists import ListRanks, evaluate_list_ranking, rank_in_lists, score_lists   # noqa: F401

__all__ = ["LiteralKG", "Aggregator", "Gate", "GateMul", "KGStructure", "KnownTriples", "RankResult", "evaluate_ranking",
           "TopKResult", "predict_topk", "FoldedMLPHead", "fold_mlp_head", "mlp_scores", "rank_pairs_mlp",
           "evaluate_mlp_ranking", "score_pairs_mlp", "evaluate_mlp_classification", "TripleThresholds", "score_triples",
           "fit_triple_thresholds", "evaluate_triple_classification", "RelationTopK", "score_relations", "rank_relations",
           "predict_relations", "evaluate_relation_prediction", "AcceptedResult", "predict_accepted", "count_accepted",
           "AnswerRanks", "rank_answers", "evaluate_retrieval", "one_vs_all_loss", "kvs_all_loss",
           "sigmoid_all_loss", "distinct_queries", "self_adversarial_loss", "sampled_sigmoid_loss", "group_sampled_batch",
           "NegativeSampler", "NegativeBatch", "TripleEpoch", "RelationCardinalities", "relation_cardinalities",
           "answer_counts", "subsampling_weights", "sampled_negative_loss", "relation_loss", "relation_softmax_loss",
           "gemm_ordered", "gemm_ordered_splits", "matmul_ordered", "product_route", "current_route",
           "sample_neighbors", "predict_accepted_mlp", "count_accepted_mlp", "ListRanks", "score_lists", "rank_in_lists",
           "evaluate_list_ranking"]
