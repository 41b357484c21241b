"""Generates reference_api_names.json: every camelCase member function name the reference declares in
RobotController.h, TemplateTask.h, JointTask.h and MotionForceTask.h (what
tests/test_host_config.py::test_facades_carry_every_public_member_name_of_the_reference_headers checks the facades
against). Run with the reference tree's src/ directory as the argument."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("RobotController.h", "tasks/TemplateTask.h", "tasks/JointTask.h", "tasks/MotionForceTask.h")


def main(src):
    names = {}
    for h in HEADERS:
        txt = open(os.path.join(src, h)).read()
        names[h] = sorted(set(re.findall(r"\b([a-z][a-zA-Z0-9]*[A-Z][a-zA-Z0-9]*)\s*\(", txt)))
    with open(os.path.join(HERE, "reference_api_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print({h: len(v) for h, v in names.items()})


if __name__ == "__main__":
    main(sys.argv[1])
