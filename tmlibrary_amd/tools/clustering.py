"""The clustering tool (tmlib/tools/clustering.py:28-99): k-means labels for
every mapobject of a type, from a model trained on a random subset.

The request's payload is read as the reference reads it:
``chosen_object_type`` (the mapobject type), ``selected_features`` (feature
names), ``options.k`` and ``options.method`` ("kmeans").
"""
from __future__ import annotations

import logging

import numpy as np

from tmlibrary_amd.tools.base import Classifier

logger = logging.getLogger(__name__)


class Clustering(Classifier):

    __icon__ = "CLU"
    __description__ = "Clusters mapobjects based on a set of selected features."
    __options__ = {"method": ["kmeans"]}

    #: objects the model is trained on, and objects labelled per batch
    n_train = 10**6
    n_test = 10**6

    def process_request(self, submission_id, payload):
        """Trains on at most ``n_train`` random objects of the chosen type, then
        labels all of them in batches of ``n_test`` and saves the labels under
        one registered result; returns the result's id."""
        type_name = payload["chosen_object_type"]
        features = payload["selected_features"]
        options = payload["options"]
        k, method = options["k"], options["method"]
        if method not in self.__options__["method"]:
            raise ValueError('Unknown method "%s".' % method)

        result_id = self.register_result(submission_id, type_name, result_type="ScalarToolResult",
                                         unique_labels=np.arange(k))
        train_ids = self.get_random_mapobject_subset(type_name, self.n_train)
        logger.info("train on %d objects", len(train_ids))
        model, scaler = self.train_unsupervised(
            self.load_feature_values(type_name, features, train_ids), k, method)

        for number, ids in enumerate(self.partition_mapobjects(type_name, self.n_test)):
            logger.info("label batch #%d (%d objects)", number, len(ids))
            batch = self.load_feature_values(type_name, features, ids)
            self.save_result_values(type_name, result_id, self.predict(batch, model, scaler))
        return result_id
