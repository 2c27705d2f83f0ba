"""k_render_plane mutant (profiles/render_rt/mutants.txt): (w_L, w_R) = (sl, sr), the exchange of DESIGN.md §7o left out."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'dp_weights_big(dp, x_tan, w[1], w[0])',
    'dp_weights_big(dp, x_tan, w[0], w[1])')
sub(sys.argv[1], F,
    'dp_weights_small<M>(dp, div_fmh, x_tan, w[1], w[0])',
    'dp_weights_small<M>(dp, div_fmh, x_tan, w[0], w[1])')
