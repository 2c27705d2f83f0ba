"""k_render_plane mutant (profiles/render_rt/mutants.txt): in the big-radius instantiations both views are summed with w_L
(the landing record keeps both weights)."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'wr[side] = (double)w[side] * (double)r.ra;',
    'wr[side] = (double)w[DP == kDpBig ? 0 : side] * (double)r.ra;')
