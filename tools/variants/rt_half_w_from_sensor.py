"""k_render_plane mutant (profiles/render_rt/mutants.txt): half_w from the SENSOR's width -- right whenever Wt == W."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'half_w = (float)a.Wt * 0.5f',
    'half_w = (float)a.W * 0.5f')
