"""The reference's ``pretrained.face_parsing`` surface on the HIP kernels (see ``vface_amd/parsing.py``)."""
from .face_parsing_demo import FaceParser, faceParsing_demo, init_faceParsing_pretrained_model  # noqa: F401
from .model import BiSeNet  # noqa: F401
from .resnet import Resnet18  # noqa: F401
