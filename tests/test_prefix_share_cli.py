"""--n / --share-prefix on the two command lines (argument parsing only: no device)."""


def test_run_specdec_options():
    from src.specdec.run_specdec import parse_args

    a = parse_args(["--prompt", "1 2"])
    assert a.n == 1 and not a.share_prefix
    a = parse_args(["--prompt", "1 2", "--n", "4", "--share-prefix"])
    assert a.n == 4 and a.share_prefix


def test_specdec_cli_run_options():
    from src.specdec_cli.main import build_parser

    a = build_parser().parse_args(["run", "1 2 3"])
    assert a.n == 1 and not a.share_prefix
    a = build_parser().parse_args(["run", "--n", "3", "--share-prefix", "1 2 3"])
    assert a.n == 3 and a.share_prefix
