"""Group.grouping with the reference's signature (group.py:16-66), the clustering
itself running through ot_cluster (HIP cost / centroid kernels + exact host LP).

Reference defects fixed: D3 `ot_cluster` is actually called for
'emb-ot'; D4 the cold path returns the same list-of-index-lists the cache path
returns; D10 the ragged list is saved as an object array.
"""
import os
import warnings
from os.path import abspath, exists, join

import numpy as np

from .method.utils import _dense_f32, atomic_save, kmeans, kmedoids, lpa, ot_cluster

DATA_DIR = abspath(os.environ.get('ULTRARE_DATA_DIR', join(os.getcwd(), 'data')))
SAVE_DIR = abspath(os.environ.get('ULTRARE_SAVE_DIR', join(os.getcwd(), 'result')))
DENSE_MAX_ITEMS = 256          # ure_ot_cost's widest row: up to here 'rating-ot' keeps the dense route it always had


class Group(object):
    def __init__(self, rating, dataset, user_mat=None):
        self.rating = rating  # csr_matrix (only used by the 'rating-*' variants)
        self.dataset = dataset
        self.user_mat = user_mat
        self.n_user = self.rating.shape[0] if rating is not None else (len(user_mat) if user_mat is not None else 0)
        self.n_item = self.rating.shape[1] if rating is not None and len(self.rating.shape) > 1 else 0

    def grouping(self, dataset='ml1m', n_group=2, var='emb-ot', verbose=True, data_dir=None, *, reg=1e-3):
        """reg: the entropic regulariser of the 'sinkhorn' clusterer (absolute, in squared-distance units; ignored by the others
        and not part of the cache file's name)."""
        assert n_group > 1
        label_dir = (data_dir or DATA_DIR) + '/' + dataset + '/val/' + var + str(n_group) + '.npy'

        # load the cached grouping if it exists (group.py:27-32)
        if exists(label_dir):
            return [list(map(int, g)) for g in np.load(label_dir, allow_pickle=True)]

        [trans_var, cluster_var] = var.strip().split('-')
        # 'ot' is the published path (group.py:35-45); 'kmeans' / 'bkmeans' are the comparison clusterers the
        # reference imports but never dispatches (group.py:5, utils.py:354-418): an optional addition here, as are
        # '(b)kmedoids' and '(b)lpa' (utils.py:458-611) on the euclidean distances of the embedding, streamed, and 'sinkhorn':
        # ot_cluster with entropic OT on the device in place of the exact LP (not parity: groups need not be balanced)
        assert cluster_var in ['ot', 'sinkhorn', 'kmeans', 'bkmeans', 'kmedoids', 'bkmedoids', 'lpa', 'blpa'], \
            "cluster_var must be 'ot' (published path), 'sinkhorn', 'kmeans', 'bkmeans', 'kmedoids', 'bkmedoids', 'lpa' or 'blpa'"
        if trans_var == 'rating':
            if len(self.rating.shape) != 2:
                raise ValueError(f'the rating matrix must be 2-D, not of shape {tuple(self.rating.shape)}')
            if cluster_var in ('ot', 'sinkhorn') and self.n_item > DENSE_MAX_ITEMS:
                # the CSR goes straight through: ot_cluster runs the cost and the centroid update on the sparse matrix
                # (csrc/csr_group.hip) and n_user x n_item is never formed; bad input is refused before any device work
                from .sparse_group import check_cluster_args
                embedding = check_cluster_args(self.rating, n_group)
            elif cluster_var in ('kmeans', 'bkmeans') and self.n_item > DENSE_MAX_ITEMS:
                # likewise: kmeans runs its cost, fill and centroid update on the sparse matrix (csrc/csr_kmeans.hip)
                from .sparse_kmeans import check_kmeans_args
                embedding = check_kmeans_args(self.rating, n_group)
            elif cluster_var in ('kmedoids', 'bkmedoids', 'lpa', 'blpa') and self.n_item > DENSE_MAX_ITEMS:
                # likewise: the pair distances are streamed from the sparse rows (the CSR tile producer of csrc/pair_dist.hip)
                from .sparse_pair import check_pair_args
                embedding = check_pair_args(self.rating, 'euclidean', self.n_user, n_group, 128 if cluster_var in ('lpa', 'blpa') else None)
            else:
                embedding = np.asarray(self.rating.todense(), dtype=np.float32)
        elif trans_var == 'emb':
            embedding = self.user_mat
        else:
            raise ValueError(var)
        if cluster_var == 'ot':
            _, label = ot_cluster(embedding, n_group)
        elif cluster_var == 'sinkhorn':
            _, label = ot_cluster(embedding, n_group, solver='sinkhorn', reg=reg)
        elif cluster_var in ('kmeans', 'bkmeans'):
            label = kmeans(n_group, self.n_user if isinstance(embedding, tuple) else len(embedding), embedding, balanced=cluster_var == 'bkmeans')
        elif cluster_var in ('kmedoids', 'bkmedoids'):
            X = embedding if isinstance(embedding, tuple) else _dense_f32(embedding)
            label = kmedoids(n_group, self.n_user if isinstance(X, tuple) else len(X), X, balanced=cluster_var == 'bkmedoids', metric='euclidean')
        else:
            X = embedding if isinstance(embedding, tuple) else _dense_f32(embedding)
            label = lpa(n_group, self.n_user if isinstance(X, tuple) else len(X), X, balanced=cluster_var == 'blpa', metric='euclidean')

        if verbose:
            print(''.join(str(i) + ': ' + str(int((label == i).sum())) + ', ' for i in range(n_group)))

        # labels -> index lists, ascending user id inside each list (group.py:55-58)
        res = [np.flatnonzero(label == idx).tolist() for idx in range(n_group)]

        os.makedirs(os.path.dirname(label_dir), exist_ok=True)
        arr = np.empty(n_group, dtype=object)
        for i, g in enumerate(res):
            arr[i] = g
        def write(tmp):
            with warnings.catch_warnings(), open(tmp, 'wb') as f:
                warnings.simplefilter('ignore')
                np.save(f, arr)
        atomic_save(label_dir, write)
        return res
