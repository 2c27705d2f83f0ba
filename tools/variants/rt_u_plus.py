"""k_render_plane mutant (profiles/render_rt/mutants.txt): u = half_w + px inv -- the image mirrored left to right."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'u = half_w - r.ox * a.inv_texel',
    'u = half_w + r.ox * a.inv_texel')
