"""k_render_layers_dp_grad mutant (profiles/render_dp_grad/mutants.txt): dw_L and dw_R exchanged: A_0 multiplies the derivative of s_l, A_1 that of s_r."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'acc[c] += A[0] * dwl + A[1] * dwr;',
    'acc[c] += A[0] * dwr + A[1] * dwl;')
