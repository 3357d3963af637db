"""The supervised classification tool (tmlib/tools/classification.py:27-116):
labels for every mapobject of a type from a random forest or an SVM trained on
the objects the user assigned to classes.

The request's payload is read as the reference reads it:
``chosen_object_type``, ``selected_features``, ``training_classes`` (per class
``name``, ``object_ids``, ``color``), ``options.method`` ("randomforest" or
"svm") and ``options.n_fold_cv``; an optional ``options.random_state`` seeds the
forest so that a request is repeatable.  Training runs in scikit-learn on the
host, the labelling of every object on the GPU (tools/supervised.py).
"""
from __future__ import annotations

import logging

import numpy as np

from tmlibrary_amd.tools.base import Classifier
from tmlibrary_amd.tools.supervised import train_supervised

logger = logging.getLogger(__name__)


class Classification(Classifier):

    __icon__ = "SVC"
    __description__ = ("Classifies mapobjects based on the values of selected features and "
                       "labels provided by the user.")
    __options__ = {"method": ["randomforest", "svm"], "n_fold_cv": 10}

    #: objects labelled per batch
    n_test = 10**6

    def train_supervised(self, feature_data, labels, method, n_fold_cv, random_state=None):
        """-> (model, scaler), trained on ``feature_data`` (base.py:502-584)."""
        return train_supervised(feature_data, labels, method, n_fold_cv, random_state=random_state)

    def process_request(self, submission_id, payload):
        """Trains on the objects of ``training_classes``, then labels every object
        of the chosen type in batches of ``n_test`` and saves the labels under one
        registered result; returns the result's id."""
        logger.info("perform supervised classification")
        type_name = payload["chosen_object_type"]
        features = payload["selected_features"]
        options = payload["options"]
        method, n_fold_cv = options["method"], options["n_fold_cv"]
        if method not in self.__options__["method"]:
            raise ValueError('Unknown method "%s".' % method)

        labels, label_map = {}, {}
        for i, cls in enumerate(payload["training_classes"]):
            labels.update({int(j): float(i) for j in cls["object_ids"]})
            label_map[float(i)] = {"name": cls["name"], "color": cls["color"]}
        unique_labels = np.unique(list(labels.values()))
        result_id = self.register_result(submission_id, type_name,
                                         result_type="SupervisedClassifierToolResult",
                                         unique_labels=unique_labels, label_map=label_map)

        # in ascending id, which is the order the reference's Python 2 dict of
        # small integer keys yields: KFold does not shuffle, so rows ordered by
        # class would leave folds with a single class
        training_set = self.load_feature_values(type_name, features, sorted(labels))
        logger.info("train classifier on %d objects", len(training_set))
        model, scaler = self.train_supervised(training_set, labels, method, n_fold_cv,
                                              random_state=options.get("random_state"))

        for number, ids in enumerate(self.partition_mapobjects(type_name, self.n_test)):
            logger.info("predict labels for batch #%d (%d objects)", number, len(ids))
            batch = self.load_feature_values(type_name, features, ids)
            self.save_result_values(type_name, result_id, self.predict(batch, model, scaler))
        return result_id
