"""Data-analysis tools (tmlib/tools): the clustering tool."""
from tmlibrary_amd.tools.base import (Classifier, FeatureStore, KMeans,  # noqa: F401
                                      RobustScaler, Tool)
from tmlibrary_amd.tools.clustering import Clustering  # noqa: F401
