"""Data-analysis tools (tmlib/tools): the clustering and the classification tool."""
from tmlibrary_amd.tools.base import (Classifier, FeatureStore, KMeans,  # noqa: F401
                                      RobustScaler, Tool)
from tmlibrary_amd.tools.classification import Classification  # noqa: F401
from tmlibrary_amd.tools.clustering import Clustering  # noqa: F401
from tmlibrary_amd.tools.supervised import (ForestModel, SVCModel,  # noqa: F401
                                            train_supervised)
