"""operator namespace (mirrors epgpy/operators.py:1-25, hot-path subset)"""
from .operator import (Operator, MultiOperator, EmptyOperator, Spoiler, Wait, Offset, Reset, PD,
                       NULL, SPOILER, RESET, System)
from .probe import Probe, Adc, ADC, DFT, Imaging
from .opmatrix import MatrixOp
from .opscalar import ScalarOp
from .evolution import E, P, R
from .transition import T, Tx, Ty, Phi
from .shift import S, G, C
from .diffusion import D
from .diff import Jacobian, Hessian, PartialsPruner
from .exchange import X
from .rfpulse import RFPulse
