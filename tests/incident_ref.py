"""Reference of the ic stream's rules (docs/INCIDENTS.md) for the tests: a dict per (series, source)
and plain ifs.  It shares no code with the oracle (models/oracle.py) or the engine (incidentcmp.h).

A state is {"code0", "since", "age", "hot_run", "clear_run"}; code0 "" means closed.  ``code`` is
this rollover's code of the source, "" when the source is not hot for the series (or the series has
no st row)."""

SOURCES = ("sb", "tf", "po", "ls")


def new_state():
    return {"code0": "", "since": 0, "age": 0, "hot_run": 0, "clear_run": 0}


def step(st, code, edge_ts, open_after, close_after, remind_every):
    """One rollover of one state, in place.  Returns None, or what the row prints:
    (event, code0, code or "-", since, age, run)."""
    hot = code != ""
    if hot:
        st["hot_run"] = st["hot_run"] + 1
        if st["hot_run"] > 255:
            st["hot_run"] = 255
        st["clear_run"] = 0
    else:
        st["clear_run"] = st["clear_run"] + 1
        if st["clear_run"] > 255:
            st["clear_run"] = 255
        st["hot_run"] = 0
    run = st["hot_run"] if hot else st["clear_run"]
    shown = code if hot else "-"
    if st["code0"] == "":
        if hot and st["hot_run"] >= open_after:
            st["code0"] = code
            st["since"] = edge_ts
            st["age"] = 0
            return ("O", code, shown, edge_ts, 0, run)
        return None
    st["age"] = st["age"] + 1
    if st["age"] > 2 ** 32 - 1:
        st["age"] = 2 ** 32 - 1
    if not hot and st["clear_run"] >= close_after:
        row = ("C", st["code0"], shown, st["since"], st["age"], run)
        st["code0"] = ""
        return row
    if remind_every != 0 and st["age"] % remind_every == 0:
        return ("S", st["code0"], shown, st["since"], st["age"], run)
    return None


def code_of(source, word):
    """The code a source's verdict word stands for ("" = not hot): sb any rule fired; tf / ls two
    bits a rule, rule 0 lowest, 1 = D / U and 2 = S / D, the lowest-numbered rule that is not 0;
    po 1 = H, 2 = L."""
    if source == "sb":
        return "B" if word != 0 else ""
    if source == "po":
        if word == 1:
            return "H"
        if word == 2:
            return "L"
        return ""
    for j in range(4):
        v = (word >> (2 * j)) & 3
        if v == 1:
            return "D" if source == "tf" else "U"
        if v == 2:
            return "S" if source == "tf" else "D"
    return ""


def row_text(edge_ts, server, service, source, row):
    event, code0, shown, since, age, run = row
    return f"ic|{edge_ts}|{server}|{service}|{source}|{event}|{code0}|{shown}|{since}|{age}|{run}"


class Book:
    """The states of many series: step_all runs one rollover and returns the rows in the order given."""

    def __init__(self, sources, remind_every=0):
        self.sources = dict(sources)      # source -> (open_after, close_after)
        self.remind_every = remind_every
        self.states = {}                  # (series key, source) -> state

    def step_all(self, edge_ts, series):
        """``series``: [(key, server, service, {source: code})] in emission order; a series without an
        st row carries an empty dict.  Returns the rows' text."""
        out = []
        for key, server, service, codes in series:
            for src in SOURCES:
                if src not in self.sources:
                    continue
                st = self.states.setdefault((key, src), new_state())
                oa, ca = self.sources[src]
                row = step(st, codes.get(src, ""), edge_ts, oa, ca, self.remind_every)
                if row is not None:
                    out.append(row_text(edge_ts, server, service, src, row))
        return out

    def open_count(self, source):
        return sum(1 for (k, s), st in self.states.items() if s == source and st["code0"] != "")
