from egopose_amd.agent import AgentVGAIL  # noqa: F401
