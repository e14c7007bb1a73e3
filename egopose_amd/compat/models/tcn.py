from egopose_amd.tcn import TemporalConvNet  # noqa: F401
