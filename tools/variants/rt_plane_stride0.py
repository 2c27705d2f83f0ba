"""k_render_plane mutant (profiles/render_rt/mutants.txt): k * plane replaced by 0 -- every plane of a launch reads its first."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'a.tex + k * plane;',
    'a.tex + 0 * plane;')
