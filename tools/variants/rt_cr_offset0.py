"""k_render_plane mutant (profiles/render_rt/mutants.txt): the right tap column taken with offset 0 (cr = cl)."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'cr = clamped_texel(c0, 1, a.Wt)',
    'cr = clamped_texel(c0, 0, a.Wt)')
