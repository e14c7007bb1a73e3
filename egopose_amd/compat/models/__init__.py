from .mlp import MLP  # noqa: F401
from .rnn import RNN  # noqa: F401
from .tcn import TemporalConvNet  # noqa: F401
from .resnet import ResNet  # noqa: F401
