"""The synthetic chain of the va stage's cdof-stack tests (test_va_lds_cpu.py, test_va_lds_gpu.py).

A free joint, a ball joint, a slide and eleven hinges in series, with a short side branch so
that a slot is reused after its first owner's post-visit. The deepest path has 3 + 3 + 1 + 11
= 18 non-constant dofs (the free joint's three translations are literals and take no slot),
more than the 9 slots that fit the LDS budget beside this model's 21-dof output block, so the
tree pass takes both the slot branch and the re-read branch.
"""
from mujoco_inversedynamicstest_amd import mjcf

NHINGE = 11


def chain_xml(nhinge=NHINGE):
  axes = ("1 0 0", "0 1 0", "0 0 1", "1 1 0", "0 1 1")
  body = ""
  for h in reversed(range(nhinge)):
    side = ('<body pos="0 .05 0"><joint name="side" axis="0 0 1" damping=".05"/>'
            '<geom size=".02" pos="0 .04 0"/></body>') if h == 2 else ""
    body = (f'<body pos=".1 0 {0.01 * h}"><joint name="h{h}" axis="{axes[h % len(axes)]}" '
            f'damping="{0.1 + 0.01 * h}" stiffness="{0.5 * (h % 3)}" armature=".01"/>'
            f'<geom type="capsule" fromto="0 0 0 .1 0 0" size=".02"/>{side}{body}</body>')
  return f"""<mujoco><option><flag contact="disable"/></option><worldbody>
    <body pos="0 0 1"><freejoint/><geom type="box" size=".1 .08 .05"/>
      <body pos=".15 0 0"><joint name="ball" type="ball" damping=".2" stiffness="1"/>
        <geom type="capsule" fromto="0 0 0 .2 0 0" size=".03"/>
        <body pos=".2 0 0"><joint name="slide" type="slide" axis="1 0 1" damping=".3"/>
          <geom size=".04"/>{body}</body></body></body>
    </worldbody></mujoco>"""


def load():
  return mjcf.load_xml_string(chain_xml())
