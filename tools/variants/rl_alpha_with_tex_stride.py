"""k_render_layers mutant (profiles/render_layers/mutants.txt): the coverage follows the colour's layer stride -- a shared image
(stride 0) reads layer 0's coverage on every layer.  The in-range form of "alpha + l * layer_stride", which would leave the
coverage array whenever a layer has more than one colour plane."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'taps.read(a.alpha + l * plane);',
    'taps.read(a.alpha + (a.layer_stride ? l : 0) * plane);')
