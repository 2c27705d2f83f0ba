"""k_render_plane mutant (profiles/render_rt/mutants.txt): the bilinear weights w01 and w10 exchanged."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'w01 = (1.0 - dv) * du, w10 = dv * (1.0 - du)',
    'w01 = dv * (1.0 - du), w10 = (1.0 - dv) * du')
