"""A numbered section of a profile under profiles/ whose figures a tool writes itself: the lines between the section's underlined heading
and its "Reading." paragraph are the tool's output, the rest of the file is prose that stays."""
import contextlib
import io
import sys


class Tee(io.StringIO):
    def write(self, s):
        sys.__stdout__.write(s)
        return super().write(s)

    def flush(self):
        sys.__stdout__.flush()


def write_section(path, number, text):
    lines = open(path).read().split("\n")
    head = next(i for i, l in enumerate(lines[:-1]) if l.startswith("%d. " % number) and lines[i + 1] and set(lines[i + 1]) == {"="})
    end = next(i for i in range(head + 2, len(lines)) if lines[i].startswith("Reading."))
    lines[head + 2:end] = text.rstrip("\n").split("\n") + [""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


@contextlib.contextmanager
def section(path, number):
    """Everything printed inside goes to stdout and, where `path` is given, becomes section `number` of that file."""
    tee = Tee()
    with contextlib.redirect_stdout(tee):
        yield
    if path:
        write_section(path, number, tee.getvalue())
